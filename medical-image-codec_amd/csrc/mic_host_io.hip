// mic_host_io.hip -- the entry points a cgo caller uses: host buffers in, host buffers out.
//
// The reference hands Go slices to its C codec (ojph/mic_c.go:26-39, :169-185) and fans strips / frames out over goroutines
// (parallelstrips.go:77-93, multiframecompress.go:201-203).  Here a call
//   * leases a session of the default pool (mic_api.hip: concurrent callers run on different sessions),
//   * cuts its units into sub-batches and runs them as a three-stage pipeline -- sub-batch k + 1 comes up over PCIe while k is
//     coded and k - 1 goes down -- with two halves of every staging buffer (run_staged, mic_staged.h: the one place that does),
//   * moves bytes through the transfer engine below: a caller's buffer is ordinary pageable memory (a Go slice), which the
//     runtime can only DMA through its own small bounce buffer; a handful of worker threads copy 4 MiB chunks into pinned slots
//     and DMA them on their own streams, so the link stays busy.  Memory from mic_hip_host_alloc (or any registered memory) is
//     pinned already and is DMA-ed in place.
// There is no CPU codec here: the host copies bytes and writes container headers.
#include "mic_session.h"
#include "mic_staged.h"
#include <chrono>
#include <climits>

#include <atomic>
#include <deque>
#include <thread>

namespace {

// ============================================================================ transfer engine
constexpr size_t kChunk = (size_t)4 << 20;        // bytes per pinned slot
constexpr size_t kDirectChunk = (size_t)64 << 20; // pinned user memory: pieces this large, spread over the workers' streams
constexpr size_t kInline = (size_t)128 << 10;     // pageable transfers up to this size: a plain hipMemcpy on the calling thread

struct IoChunk { IoReq *req; int device; void *dev; void *host; size_t bytes; bool to_device; bool direct; };

bool host_is_pinned(const void *p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

class IoPool {
public:
    static IoPool &get() { static IoPool p; return p; }
    void push(const IoChunk &c) {
        { std::lock_guard<std::mutex> lk(mu_); q_[c.to_device ? 0 : 1].push_back(c); }
        cv_.notify_all();
    }
    int threads() const { return (int)th_.size(); }
private:
    struct Slot { void *pin = nullptr; hipEvent_t ev = nullptr; bool busy = false; IoReq *req = nullptr; void *host_dst = nullptr; size_t bytes = 0; };
    struct PerDev { hipStream_t st = nullptr; Slot slot[2]; int next = 0; bool ok = false; };
    std::vector<std::thread> th_;
    std::deque<IoChunk> q_[2];                     // uploads, downloads: half the workers look at one first, half at the other, so a
                                                   // download queued behind a long upload starts at once and the link runs both ways
    std::mutex mu_; std::condition_variable cv_;
    bool stop_ = false;

    IoPool() {
        const char *e = getenv("MIC_HIP_IO_THREADS");
        int n = e ? atoi(e) : 0;
        if (n <= 0) n = (int)std::min<unsigned>(8u, std::max<unsigned>(2u, std::thread::hardware_concurrency() / 2));
        n = std::min(n, 32);
        for (int i = 0; i < n; i++) th_.emplace_back([this, i] { run(i & 1); });
    }
    ~IoPool() {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_.notify_all();
        for (auto &t : th_) if (t.joinable()) t.join();
    }
    static void retire(Slot &s, bool ok = true) {
        if (!s.busy) return;
        ok = ok && hipEventSynchronize(s.ev) == hipSuccess;
        if (ok && s.host_dst) memcpy(s.host_dst, s.pin, s.bytes);
        s.busy = false;
        s.req->done(ok);
    }
    // a slot whose transfer has completed is retired at once -- its request is signalled (and a pageable download copied out) before
    // the worker takes more work: waiting for the slot's next use held a request's last chunks back for two more submissions, and
    // with callers on several devices for as long as the other device's request kept the worker fed
    static void retire_finished(Slot &s) {
        if (!s.busy) return;
        const hipError_t e = hipEventQuery(s.ev);
        if (e == hipErrorNotReady) (void)hipGetLastError();   // (not an error to keep)
        else retire(s, e == hipSuccess);                      // (any other failure is the slot's transfer's)
    }
    void run(int first) {
        std::vector<PerDev> devs;
        for (;;) {
            IoChunk c;
            bool have = false;
            for (auto &d : devs) { retire_finished(d.slot[0]); retire_finished(d.slot[1]); }
            {
                std::unique_lock<std::mutex> lk(mu_);
                bool inflight = false;
                for (auto &d : devs) inflight |= d.slot[0].busy || d.slot[1].busy;
                auto none = [&] { return q_[0].empty() && q_[1].empty(); };
                if (none() && !inflight && !stop_) cv_.wait(lk, [&] { return stop_ || !none(); });
                std::deque<IoChunk> &q = !q_[first].empty() ? q_[first] : q_[first ^ 1];
                if (!q.empty()) { c = q.front(); q.pop_front(); have = true; }
                else if (stop_ && !inflight) return;
            }
            if (!have) {                                   // nothing new: finish what is in flight
                for (auto &d : devs) { retire(d.slot[0]); retire(d.slot[1]); }
                continue;
            }
            if ((int)devs.size() <= c.device) devs.resize((size_t)c.device + 1);
            PerDev &d = devs[(size_t)c.device];
            bool ok = hipSetDevice(c.device) == hipSuccess;
            if (ok && !d.ok) {
                // a stream of the HIGHEST priority: the runtime keeps a hardware queue per priority level, and a transfer on an
                // ordinary stream can land on the queue the session's kernels sit in and wait behind them (seen: the upload of
                // sub-batch k + 1 and the download of k - 1 only made progress between two decodes)
                int lo = 0, hi = 0;
                (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
                ok = hipStreamCreateWithPriority(&d.st, hipStreamNonBlocking, hi) == hipSuccess;
                for (int i = 0; ok && i < 2; i++)
                    ok = hipHostMalloc(&d.slot[i].pin, kChunk, hipHostMallocDefault) == hipSuccess &&
                         hipEventCreateWithFlags(&d.slot[i].ev, hipEventDisableTiming) == hipSuccess;
                d.ok = ok;
            }
            if (!ok) { c.req->done(false); continue; }
            Slot &s = d.slot[d.next]; d.next ^= 1;
            retire(s);                                     // (its DMA had the other slot's copy to complete in)
            hipError_t e;
            if (c.direct) {
                e = hipMemcpyAsync(c.to_device ? c.dev : c.host, c.to_device ? c.host : c.dev, c.bytes,
                                   c.to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, d.st);
                s.host_dst = nullptr;
            } else if (c.to_device) {
                memcpy(s.pin, c.host, c.bytes);
                e = hipMemcpyAsync(c.dev, s.pin, c.bytes, hipMemcpyHostToDevice, d.st);
                s.host_dst = nullptr;
            } else {
                e = hipMemcpyAsync(s.pin, c.dev, c.bytes, hipMemcpyDeviceToHost, d.st);
                s.host_dst = c.host;
            }
            if (e == hipSuccess) e = hipEventRecord(s.ev, d.st);
            if (e != hipSuccess) { c.req->done(false); continue; }
            s.busy = true; s.req = c.req; s.bytes = c.bytes;
        }
    }
};

// One host <-> device transfer, joined to `req`.  The device side must be ready when this is called (uploads: the target is
// not in use; downloads: the producing stream has been synchronised) and is complete after req.wait().
int io_submit(IoReq &req, int device, void *dev, const void *host, size_t bytes, bool to_device) {
    if (bytes == 0) return MIC_OK;
    void *h = const_cast<void *>(host);
    const bool pinned = host_is_pinned(host);
    if (!pinned && bytes <= kInline) {
        HIP_TRY(to_device ? hipMemcpy(dev, h, bytes, hipMemcpyHostToDevice) : hipMemcpy(h, dev, bytes, hipMemcpyDeviceToHost));
        return MIC_OK;
    }
    IoPool &pool = IoPool::get();
    const size_t step = pinned ? kDirectChunk : kChunk;
    const int n = (int)((bytes + step - 1) / step);
    req.add(n);
    for (int i = 0; i < n; i++) {
        const size_t off = (size_t)i * step, len = std::min(step, bytes - off);
        pool.push(IoChunk{ &req, device, (char *)dev + off, (char *)h + off, len, to_device, pinned });
    }
    return MIC_OK;
}

// ============================================================================ pipelined unit codec over host buffers
// A GROUP is what one destination buffer receives (a job, a PICS image, a MIC2 stack); its units are consecutive, their pixels
// lie back to back in the group's host buffer, their streams go back to back behind `hdr` bytes of the group's output.
struct DestRun {                                      // the run of streams a destination buffer receives behind its `hdr` bytes
    uint8_t *out; size_t cap, hdr;
    size_t written = 0; bool cap_fail = false;        // cap_fail: the run did not fit (the owner reports MIC_ERR_CAPACITY and appends no more)
    // the next `bytes` of the run, from device memory that is ready (io_submit): queued on `down`, or the run is marked as too long
    int append(IoReq &down, int device, const uint8_t *d_src, size_t bytes) {
        if (hdr + written + bytes > cap) { cap_fail = true; return MIC_OK; }
        const int rc = io_submit(down, device, const_cast<uint8_t *>(d_src), out + hdr + written, bytes, false);
        written += bytes;
        return rc;
    }
};
// session_encode_finish has left a chain's streams in s->packed: they stay there while the next chain packs into the other half, which
// the download `prev` (of the chain before; null: none) may still be reading
inline int keep_packed(mic_hip_session *s, IoReq *prev) {
    const int rc = prev ? prev->wait() : MIC_OK;
    if (rc == MIC_OK) std::swap(s->packed, s->packed2);
    return rc;
}
struct EncGroup {
    const uint16_t *h_px; DestRun dst;
    int first, n;
    int32_t status = MIC_OK;
    int failed = -1;                                  // the group's first unit that failed, counted from `first` ("strip %d", parallelstrips.go:97)
};
struct EncUnit {
    uint64_t px_off; int32_t w, h; uint16_t maxv, nstates; int group;
    int32_t status = MIC_OK, nstates_used = 0; size_t len = 0;
    mic_hip_verify_result vr{ MIC_OK, 0, 0, -1 };     // the verified doors: what the check of this unit's stream said
};
struct DecGroup {
    const uint8_t *h_comp; uint16_t *h_px;
    int first, n;
    int32_t status = MIC_OK;
    int failed = -1;
};
struct DecUnit {
    size_t comp_off, comp_len; uint64_t px_off; int32_t w, h; uint16_t flags; int group;
    int32_t status = MIC_OK;
    uint32_t crc = 0;                                 // the _crc doors: CRC-32 of the unit's decoded pixels
};

inline bool unit_gap(const EncUnit &u) { return (u.nstates & MIC_HIP_GAP_REMOVAL) != 0; }
inline bool unit_gap(const DecUnit &u) { return (u.flags & MIC_HIP_GAP_REMOVAL) != 0; }
// units [i0, i1) of the next sub-batch of units [.., n): under the workspace ceiling, and -- when the call is large enough to be worth a pipeline --
// about `target` units (the kernels want a couple of thousand units per launch: the tANS decode chain takes as long for ten
// streams as for 2304)
// staging: bytes per pixel a unit holds beside its slabs -- two halves each of the pixels, the streams, the packed buffer; the verified
// encode adds the pixels its streams decode to
template <class U>
int next_cut(const std::vector<U> &units, int i0, int n, size_t target, size_t staging = 12) {
    size_t max_px = 0, gap_x = 0, cap = 0;
    return (int)next_sub_batch((size_t)i0, (size_t)n, [&](size_t i) { return (size_t)units[i].w * (size_t)units[i].h; }, [&](size_t i, size_t mp) {
        // (a gap-removal unit holds a map slab beside the others: the tier-2 one is counted)
        const size_t gx = std::max(gap_x, unit_gap(units[i]) ? (size_t)mic_gap_stride(65536u) : (size_t)0);
        if (mp != max_px || gx != gap_x || cap == 0) cap = batch_units_for(mp, 1, staging * mp + gx);
        max_px = mp; gap_x = gx;
        return cap;
    }, CutRule{ 65535, target });
}
// Sub-batches of a call: the transfers of one overlap the kernels of its neighbours.  A decode costs the tANS chain's ~17 ms whatever
// its size (one serial chain per stream), so decode cuts into parts of >= 1152 units; encode kernels scale with their units (7 ms
// for 2304), so encode cuts into parts of >= 768 -- three at most either way: measured on 2304 strips in pinned buffers, encode /
// decode with 2 parts 75 / 92 ms (decode's default), 3 parts 78 / 94 (encode's default: 75 with decode at 2), 4 parts 88 / 106.
inline size_t pipeline_target(size_t n_units, bool encode) {
    const size_t min_units = encode ? 768 : 1152, max_parts = 3;
    static const char *ov = getenv("MIC_HIP_PIPELINE_PARTS");              // (experiments: force the number of parts)
    size_t parts = ov ? (size_t)std::max(1, atoi(ov)) : std::min(max_parts, n_units / min_units);
    if (parts < 2) return n_units ? n_units : 1;
    return (n_units + parts - 1) / parts;
}

// Groups [g0, g1) of the call -- their units are one range of U -- on session s; G and U are the caller's, every index is the call's.
// verify: every sub-batch's packed streams are decoded again and compared with its pixels, both still on the device (session_verify);
// U[i].vr says what came of it.  Nothing else changes: a unit that fails the check is delivered like any other.
int encode_groups(mic_hip_session *s, std::vector<EncGroup> &G, std::vector<EncUnit> &U, int g0, int g1, bool verify = false) {
    if (g0 >= g1) return MIC_OK;
    const int u0 = G[(size_t)g0].first, n = G[(size_t)g1 - 1].first + G[(size_t)g1 - 1].n;
    if (u0 == n) return MIC_OK;
    const size_t target = pipeline_target((size_t)(n - u0), true);
    struct Sub { int i0, i1; std::vector<mic_hip_unit> units; size_t px; };
    const std::vector<Sub> subs = staged_cut<Sub>(u0, n, [&](int i0) { return next_cut(U, i0, n, target, verify ? 14 : 12); }, [&](int i0, int i1) {
        Sub sb{ i0, i1, std::vector<mic_hip_unit>((size_t)(i1 - i0)), 0 };
        for (int i = i0; i < i1; i++) {
            const EncUnit &u = U[(size_t)i];
            sb.units[(size_t)(i - i0)] = mic_hip_unit{ sb.px, u.w, u.h, u.maxv, u.nstates };
            sb.px += (size_t)u.w * (size_t)u.h;
        }
        return sb;
    });
    for (size_t k = 0; k < subs.size(); k++) trace_part("units encode", k, subs.size(), "units", subs[k].i0, subs[k].i1, subs[k].px);
    DevBuf *in[2] = { &s->io_px, &s->io_px2 };
    IoReq *prev = nullptr;                                // the download of the part before: keep_packed waits for it
    return run_staged(subs.size(), [&](size_t k, int half, IoReq &up) -> int {
        const Sub &sb = subs[k];
        int r = in[half]->reserve(sb.px * 2 + 64);
        if (r) return r;
        // one transfer per run of units that are neighbours in one host buffer
        size_t doff = 0;
        for (int i = sb.i0; i < sb.i1;) {
            const EncGroup &g = G[(size_t)U[(size_t)i].group];
            int j = i; size_t run = 0;
            while (j < sb.i1 && U[(size_t)j].group == U[(size_t)i].group && U[(size_t)j].px_off == U[(size_t)i].px_off + run) {
                run += (size_t)U[(size_t)j].w * (size_t)U[(size_t)j].h; j++;
            }
            if ((r = io_submit(up, s->device, (uint16_t *)in[half]->p + doff, g.h_px + U[(size_t)i].px_off, run * 2, true))) return r;
            doff += run; i = j;
        }
        return MIC_OK;
    }, [&](size_t k, int half, IoReq &down, IoReq *) -> int {
        const Sub &sb = subs[k];
        const int nb = sb.i1 - sb.i0;
        std::vector<uint64_t> offs((size_t)nb + 1); std::vector<int32_t> st((size_t)nb), ns((size_t)nb);
        const uint8_t *d_blobs = nullptr;
        int rc = session_encode_enqueue(s, (const uint16_t *)in[half]->p, sb.units.data(), nb);
        if (rc == MIC_OK) rc = session_encode_finish(s, &d_blobs, offs.data(), st.data(), ns.data());
        if (rc == MIC_OK && verify) {                      // (the pixels are still in this half, the streams in s->packed)
            std::vector<mic_hip_verify_result> vr((size_t)nb);
            rc = session_verify(s, d_blobs, offs.data(), offs.data() + 1, sb.units.data(), nb, (const uint16_t *)in[half]->p, st.data(), vr.data());
            for (int i = sb.i0; i < sb.i1 && rc == MIC_OK; i++) U[(size_t)i].vr = vr[(size_t)(i - sb.i0)];
        }
        if (rc == MIC_OK) rc = keep_packed(s, prev);
        if (rc != MIC_OK) return rc;
        prev = &down;
        for (int i = sb.i0; i < sb.i1;) {                  // per group: its streams of this sub-batch, one transfer
            EncGroup &g = G[(size_t)U[(size_t)i].group];
            int j = i;
            while (j < sb.i1 && U[(size_t)j].group == U[(size_t)i].group) j++;
            size_t bytes = 0;
            for (int q = i; q < j; q++) {
                EncUnit &u = U[(size_t)q];
                u.status = st[(size_t)(q - sb.i0)]; u.nstates_used = ns[(size_t)(q - sb.i0)];
                u.len = (size_t)(offs[(size_t)(q - sb.i0) + 1] - offs[(size_t)(q - sb.i0)]);
                if (u.status != MIC_OK && g.status == MIC_OK) { g.status = u.status; g.failed = q - g.first; }   // the first failing unit names the error
                bytes += u.len;
            }
            if (g.status == MIC_OK) {
                rc = g.dst.append(down, s->device, d_blobs + offs[(size_t)(i - sb.i0)], bytes);
                if (g.dst.cap_fail) g.status = MIC_ERR_CAPACITY;
                if (rc) return rc;
            }
            i = j;
        }
        return MIC_OK;
    });
}

// digest: U[i].crc = the CRC-32 of every unit's decoded pixels, taken on the device in front of the download
int decode_groups(mic_hip_session *s, std::vector<DecGroup> &G, std::vector<DecUnit> &U, int g0, int g1, bool digest = false) {
    if (g0 >= g1) return MIC_OK;
    const int u0 = G[(size_t)g0].first, n = G[(size_t)g1 - 1].first + G[(size_t)g1 - 1].n;
    if (u0 == n) return MIC_OK;
    const size_t target = pipeline_target((size_t)(n - u0), false);
    struct Sub { int i0, i1; std::vector<mic_hip_unit> units; std::vector<uint64_t> begins, ends; size_t px; };
    std::vector<Sub> subs = staged_cut<Sub>(u0, n, [&](int i0) { return next_cut(U, i0, n, target); }, [&](int i0, int i1) {
        const size_t nb = (size_t)(i1 - i0);
        Sub sb{ i0, i1, std::vector<mic_hip_unit>(nb), std::vector<uint64_t>(nb), std::vector<uint64_t>(nb), 0 };
        for (int i = i0; i < i1; i++) {
            const DecUnit &u = U[(size_t)i];
            sb.units[(size_t)(i - i0)] = mic_hip_unit{ sb.px, u.w, u.h, 0, u.flags };
            sb.px += (size_t)u.w * (size_t)u.h;
        }
        return sb;
    });
    for (size_t k = 0; k < subs.size(); k++) trace_part("units decode", k, subs.size(), "units", subs[k].i0, subs[k].i1, subs[k].px);
    DevBuf *in[2] = { &s->io_comp, &s->io_comp2 }, *outb[2] = { &s->io_px, &s->io_px2 };
    // MIC_HIP_TRACE=1: the stages of the pipeline with their wall times on stderr (tools/: where a call's time goes)
    const auto t0 = std::chrono::steady_clock::now();
    auto mark = [&](const char *what, size_t k) {
        if (io_trace()) fprintf(stderr, "[mic_hip decode] %7.2f ms  %s %zu\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), what, k);
    };
    const int rc = run_staged(subs.size(), [&](size_t k, int half, IoReq &up) -> int {
        Sub &sb = subs[k];
        // device layout: every run of streams that are neighbours in one host buffer keeps its shape, runs start 16-byte aligned
        size_t coff = 0;
        struct Run { size_t dev, host_off, len; const uint8_t *base; };
        std::vector<Run> runs;
        for (int i = sb.i0; i < sb.i1;) {
            const int gi = U[(size_t)i].group;
            const size_t start = U[(size_t)i].comp_off;
            size_t end = start;
            int j = i;
            while (j < sb.i1 && U[(size_t)j].group == gi && U[(size_t)j].comp_off >= end && U[(size_t)j].comp_off - end <= 64) {
                sb.begins[(size_t)(j - sb.i0)] = coff + (U[(size_t)j].comp_off - start);
                sb.ends[(size_t)(j - sb.i0)] = sb.begins[(size_t)(j - sb.i0)] + U[(size_t)j].comp_len;
                end = U[(size_t)j].comp_off + U[(size_t)j].comp_len; j++;
            }
            runs.push_back(Run{ coff, start, end - start, G[(size_t)gi].h_comp });
            coff += align_up(end - start, 16);
            i = j;
        }
        int r = in[half]->reserve(coff + 64);
        if (r) return r;
        for (const Run &q : runs)
            if ((r = io_submit(up, s->device, (uint8_t *)in[half]->p + q.dev, q.base + q.host_off, q.len, true))) return r;
        return MIC_OK;
    }, [&](size_t k, int half, IoReq &down, IoReq *) -> int {
        const Sub &sb = subs[k];
        // (this sub-batch decodes into the pixel half that sub-batch k - 2 was downloaded from)
        mark("streams on the device", k);
        if (k >= 2) mark("pixels of sub-batch on the host", k - 2);
        int rc = outb[half]->reserve(sb.px * 2 + 64);
        const int nb = sb.i1 - sb.i0;
        std::vector<int32_t> st((size_t)nb);
        if (rc == MIC_OK) rc = session_decode_enqueue_spans(s, (const uint8_t *)in[half]->p, sb.begins.data(), sb.ends.data(), sb.units.data(), nb, (uint16_t *)outb[half]->p);
        if (rc == MIC_OK) rc = session_decode_finish(s, st.data());
        mark("decoded", k);
        if (rc == MIC_OK && digest) {                      // (a unit that failed to decode is hashed too -- its pixels lie inside the half -- and not reported)
            std::vector<mic_hip_verify_result> vr((size_t)nb);
            rc = session_digest_run(s, (const uint16_t *)outb[half]->p, nullptr, sb.units.data(), nb, nullptr, vr.data());
            for (int i = sb.i0; i < sb.i1 && rc == MIC_OK; i++) U[(size_t)i].crc = vr[(size_t)(i - sb.i0)].crc32;
            mark("digests", k);
        }
        if (rc != MIC_OK) return rc;
        for (int i = sb.i0; i < sb.i1;) {
            DecGroup &g = G[(size_t)U[(size_t)i].group];
            int j = i;
            while (j < sb.i1 && U[(size_t)j].group == U[(size_t)i].group) j++;
            for (int q = i; q < j; q++) {
                U[(size_t)q].status = st[(size_t)(q - sb.i0)];
                if (U[(size_t)q].status != MIC_OK && g.status == MIC_OK) { g.status = U[(size_t)q].status; g.failed = q - g.first; }
            }
            if (g.status == MIC_OK) {                      // runs of units whose pixels are neighbours in the host buffer
                for (int q = i; q < j;) {
                    int e = q; size_t run = 0;
                    while (e < j && U[(size_t)e].px_off == U[(size_t)q].px_off + run) { run += (size_t)U[(size_t)e].w * (size_t)U[(size_t)e].h; e++; }
                    if ((rc = io_submit(down, s->device, (uint16_t *)outb[half]->p + sb.units[(size_t)(q - sb.i0)].px_offset, g.h_px + U[(size_t)q].px_off, run * 2, false))) return rc;
                    q = e;
                }
            }
            i = j;
        }
        return MIC_OK;
    });
    mark("all pixels on the host", subs.size());
    return rc;
}

// ============================================================================ several devices
// mic_hip_set_devices lists the GPUs the batch entry points may use.  A call's items (groups, jobs, frames, tile rows) are cut into
// one CONTIGUOUS shard per listed device, balanced by pixels -- the static assignment of the reference's fan-outs
// (parallelstrips.go:77-93, multiframecompress.go:186-209, wsicompress.go:126-145) -- and micapi::over_devices below runs the shards
// side by side, each on a thread of its own with a session of its device's pool, its own sub-batch pipeline and the transfer engine's
// per-device streams and pinned slots.  Every shard works on the caller's own tables with the call's indices and its results go
// straight into the caller's buffers: the caller's memory is what a rank-0 view would be, there is no gather.  (A device may be
// listed twice: two shards, two sessions of one GPU.)

// what the fan-out weighs a group by: its pixels
template <class Grp, class Unt>
uint64_t group_px(const Grp &g, const std::vector<Unt> &U) {
    uint64_t px = 0;
    for (int q = g.first; q < g.first + g.n; q++) px += (uint64_t)U[(size_t)q].w * (uint64_t)U[(size_t)q].h;
    return px;
}

// the strips of a PICS image (parallelstrips.go:59-72)
inline void pics_geometry(int height, int num_strips, int &strip_h, int &actual) {
    if (num_strips > height) num_strips = height;                    // :62-67
    strip_h = (height + num_strips - 1) / num_strips;                // :70
    actual = (height + strip_h - 1) / strip_h;                       // :72
}


// ============================================================================ PICA: many images, boundaries and pick on the device
// A PICA image's units are not known before its pixels are on the device: the strip boundaries follow the content.  So the call is
// cut into PARTS of whole images (about as many units as a PICS sub-batch holds, pixels inside a staging half); a part's pixels
// come up once, k_pica_rowcost / k_pica_partition find the boundaries of all its images, one small read-back brings them to the
// host, and the strips -- two units each over the same pixels, avg and gradient -- run as launch chains under the workspace
// ceiling.  The boundary stage of part k + 1 is queued BEHIND the last chain of part k, before the host waits for that chain: its
// read-back is complete at the chain's one synchronisation, and part k + 1 starts without a round trip of its own.
struct PicaRun {                                       // one job the call runs
    mic_hip_pica_enc_job *j; int n;                    // n: strips (num_strips clamped to the height, parallelstripsadaptive.go:61-66)
    std::vector<int32_t> y0, err; std::vector<uint32_t> len, flag;   // per strip; err: the strip's error (both candidates failed, no rows)
    DestRun dst;                                       // (behind the 16 + 16 n bytes of the header)
    bool failed() const { if (dst.cap_fail) return true; for (int32_t e : err) if (e != MIC_OK) return true; return false; }
};
static_assert(sizeof(MicPicaImage) == 32, "the table travels as four u64 per image");

// -DMIC_PICA_TIMING (A / B builds only, tools/bench_pica_batch.py): per-kernel device times of every PICA batch call on stderr.
// The product library has none of it.
#ifdef MIC_PICA_TIMING
struct PicaTimingScope {
    mic_hip_session *s; const char *what;
    PicaTimingScope(mic_hip_session *s_, const char *w) : s(s_), what(w) { (void)mic_hip_session_set_timing(s, 2); }
    ~PicaTimingScope() {
        const char *names[96]; float ms[96];
        const int n = mic_hip_session_last_timings(s, names, ms, 96);
        for (int i = 0; i < n; i++) fprintf(stderr, "[mic_hip pica %s] %9.4f ms  %s\n", what, ms[i], names[i]);
        (void)mic_hip_session_set_timing(s, 0);
    }
};
#endif

struct PicaPart {
    int g0 = 0, g1 = 0;
    std::vector<MicPicaImage> tab; uint32_t rows = 0, nstarts = 0; size_t px = 0;
};

// table up, costs, boundaries, boundaries down: all on the session's stream, nothing waited for
int pica_bounds_enqueue(mic_hip_session *s, PicaPart &p, const uint16_t *d_px, int half) {
    const size_t nimg = p.tab.size();
    int rc;
    if ((rc = s->pica_pin[half].reserve(4 * nimg + ((size_t)p.nstarts + 1) / 2))) return rc;
    if ((rc = s->pica_tab.reserve(sizeof(MicPicaImage) * nimg))) return rc;
    if ((rc = s->pica_cost.reserve(8 * std::max<size_t>(p.rows, 1)))) return rc;
    if ((rc = s->pica_starts.reserve(4 * (size_t)p.nstarts))) return rc;
    memcpy(s->pica_pin[half].p, p.tab.data(), sizeof(MicPicaImage) * nimg);
    HIP_TRY(hipMemcpyAsync(s->pica_tab.p, s->pica_pin[half].p, sizeof(MicPicaImage) * nimg, hipMemcpyHostToDevice, s->stream));
    s->timer.stream = s->stream;
    mic_launch_pica_bounds(d_px, (const MicPicaImage *)s->pica_tab.p, (int)nimg, p.rows, (unsigned long long *)s->pica_cost.p,
                           (int32_t *)s->pica_starts.p, s->stream, &s->timer);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s->pica_pin[half].p + 4 * nimg, s->pica_starts.p, 4 * (size_t)p.nstarts, hipMemcpyDeviceToHost, s->stream));
    return MIC_OK;
}
inline const int32_t *pica_starts_of(const mic_hip_session *s, const PicaPart &p, int half) { return (const int32_t *)(s->pica_pin[half].p + 4 * p.tab.size()); }

// an enqueued chain nobody has finished: whichever way its owner leaves, the stream is waited for first
struct QueuedChain { mic_hip_session *s; bool queued = false; ~QueuedChain() { if (queued) (void)hipStreamSynchronize(s->stream); } };

// jobs [j0, nj) of the call's J on session s
int pica_encode_run(mic_hip_session *s, std::vector<PicaRun> &J, int j0, int nj) {
    if (j0 >= nj) return MIC_OK;
    int rc = s->ensure(1, 1);                                             // (the stream)
    if (rc) return rc;
#ifdef MIC_PICA_TIMING
    PicaTimingScope timing(s, "encode");
#endif
    size_t all_units = 0;
    for (int g = j0; g < nj; g++) all_units += 2 * (size_t)J[(size_t)g].n;
    const size_t target = pipeline_target(all_units, true);
    const size_t px_cap = workspace_budget() / 16;                        // u16 per staging half: the two halves take an eighth of the ceiling each
    std::vector<PicaPart> parts;
    for (int g = j0; g < nj;) {
        PicaPart p;
        p.g0 = g;
        size_t units = 0;
        for (; g < nj; g++) {
            const mic_hip_pica_enc_job &j = *J[(size_t)g].j;
            const int n = J[(size_t)g].n;
            const size_t ipx = (size_t)j.width * (size_t)j.height;
            const uint32_t irows = (n > 1 && n < j.height) ? (uint32_t)j.height : 0u;
            if (g > p.g0 && (units >= target || p.px + ipx > px_cap || (uint64_t)p.rows + irows > 0x7FFFFFFFull || (uint64_t)p.nstarts + (uint64_t)n > 0x7FFFFFFFull)) break;
            p.tab.push_back(MicPicaImage{ (uint64_t)p.px, j.width, j.height, n, irows, p.rows, p.nstarts });
            p.px += ipx; p.rows += irows; p.nstarts += (uint32_t)n; units += 2 * (size_t)n;
        }
        p.g1 = g;
        parts.push_back(std::move(p));
    }
    for (size_t k = 0; k < parts.size(); k++) trace_part("pica encode", k, parts.size(), "images", parts[k].g0, parts[k].g1, parts[k].px);
    DevBuf *in[2] = { &s->io_px, &s->io_px2 };
    struct Strip { int job, idx; uint64_t px_off; int32_t w, rows; uint16_t maxv; };
    // one download per chain, not per part: keep_packed waits for the chain before, across parts.  Waited for below, whatever happened.
    std::vector<std::unique_ptr<IoReq>> downs;
    rc = run_staged(parts.size(), [&](size_t k, int half, IoReq &up) -> int {
        const PicaPart &p = parts[k];
        int r = in[half]->reserve(p.px * 2 + 64);
        for (int g = p.g0; g < p.g1 && r == MIC_OK; g++) {
            const mic_hip_pica_enc_job &j = *J[(size_t)g].j;
            r = io_submit(up, s->device, (uint16_t *)in[half]->p + p.tab[(size_t)(g - p.g0)].px_off, j.pixels, (size_t)j.width * (size_t)j.height * 2, true);
        }
        return r;
    }, [&](size_t k, int half, IoReq &, IoReq *next_up) -> int {
        PicaPart &p = parts[k];
        int rc;
        QueuedChain chain{ s };
        if (k == 0) {                                                   // (the later parts' boundaries rode behind the chains of the part before)
            if ((rc = pica_bounds_enqueue(s, p, (const uint16_t *)in[0]->p, 0))) return rc;
            if (hipStreamSynchronize(s->stream) != hipSuccess) return MIC_ERR_DEVICE;
        }
        // the part's strips, from the boundaries the device found
        std::vector<Strip> strips;
        const int32_t *starts = pica_starts_of(s, p, half);
        for (int g = p.g0; g < p.g1; g++) {
            PicaRun &r = J[(size_t)g];
            const MicPicaImage &im = p.tab[(size_t)(g - p.g0)];
            const int32_t *st = starts + im.start0;
            for (int i = 0; i < r.n; i++) {
                const int32_t y0 = st[i], y1 = (i + 1 < r.n) ? st[i + 1] : im.h;
                if (y0 < 0 || y0 >= im.h || y1 > im.h) return MIC_ERR_INTERNAL;
                r.y0[(size_t)i] = y0;
                // a strip of no rows (the partition clamps late boundaries to the last row, :282-284) has nothing to code: the unit
                // codec rejects it like the reference's does, in strip order with the other strips' errors
                if (y1 <= y0) { r.err[(size_t)i] = MIC_ERR_ARGS; continue; }
                if ((size_t)(y1 - y0) * (size_t)im.w > ((size_t)1 << 28)) { r.err[(size_t)i] = MIC_ERR_UNSUPPORTED; continue; }
                strips.push_back(Strip{ g, i, im.px_off + (uint64_t)y0 * (uint64_t)im.w, im.w, y1 - y0, r.j->max_value });
            }
        }
        bool next_bounds = !next_up;                                    // the next part's boundary stage is queued (or there is none)
        const int nsr = (int)strips.size();
        for (int s0 = 0; s0 < nsr || !next_bounds;) {
            // strips [s0, s1) of the next chain: two units each, under the workspace ceiling
            const int s1 = (int)next_sub_batch((size_t)s0, (size_t)nsr, [&](size_t q) { return (size_t)strips[q].w * (size_t)strips[q].rows; },
                cap_by_largest([](size_t mp) { return batch_units_for(mp, 1, 6 * mp) / 2; }),   // (+ the staging: half a strip's pixels and streams per unit, two halves each)
                CutRule{ 65534 / 2 });
            const int nb = 2 * (s1 - s0);
            std::vector<mic_hip_unit> units((size_t)nb);
            for (int q = s0; q < s1; q++) {
                const Strip &t = strips[(size_t)q];
                units[(size_t)(2 * (q - s0))] = mic_hip_unit{ t.px_off, t.w, t.rows, t.maxv, 2 };                                         // :92
                units[(size_t)(2 * (q - s0) + 1)] = mic_hip_unit{ t.px_off, t.w, t.rows, t.maxv, (uint16_t)(2 | MIC_HIP_PRED_GRAD) };     // :94
            }
            if (nb && (rc = session_encode_enqueue(s, (const uint16_t *)in[half]->p, units.data(), nb, true))) return rc;
            chain.queued = nb != 0;
            if (s1 == nsr && !next_bounds) {                              // behind the part's last chain: the next part's boundaries
                if ((rc = next_up->wait())) return rc;
                if ((rc = pica_bounds_enqueue(s, parts[k + 1], (const uint16_t *)in[half ^ 1]->p, half ^ 1))) return rc;
                next_bounds = true;
                if (!nb && hipStreamSynchronize(s->stream) != hipSuccess) return MIC_ERR_DEVICE;
            }
            if (!nb) break;
            std::vector<uint64_t> offs((size_t)nb + 1); std::vector<int32_t> st((size_t)nb), nst((size_t)nb);
            const uint8_t *d_blobs = nullptr;
            rc = session_encode_finish(s, &d_blobs, offs.data(), st.data(), nst.data());
            chain.queued = false;
            if (rc) return rc;
            if ((rc = keep_packed(s, downs.empty() ? nullptr : downs.back().get()))) return rc;
            downs.push_back(std::make_unique<IoReq>());
            for (int q = s0; q < s1;) {                                   // per image: its winners of this chain lie back to back -- one transfer
                PicaRun &r = J[(size_t)strips[(size_t)q].job];
                int e = q;
                for (; e < s1 && strips[(size_t)e].job == strips[(size_t)q].job; e++) {
                    const size_t a = (size_t)(2 * (e - s0));
#ifndef MIC_PICA_NO_PICK
                    const int pick = s->h_units[a].skip_pack ? 1 : 0;       // k_pica_pick: the avg candidate lost (:95-103)
#else                   // (A / B builds: both candidates were packed; the rule on the host, the winner fetched by a copy of its own)
                    const int pick = (st[a + 1] == MIC_OK && (st[a] != MIC_OK || offs[a + 2] - offs[a + 1] <= offs[a + 1] - offs[a])) ? 1 : 0;
#endif
                    const int idx = strips[(size_t)e].idx;
                    r.flag[(size_t)idx] = (uint32_t)pick;                   // picaFlagGradPredictor
                    r.len[(size_t)idx] = (uint32_t)(offs[a + (size_t)pick + 1] - offs[a + (size_t)pick]);
                    r.err[(size_t)idx] = pick ? st[a + 1] : st[a];          // both failed: the avg error ("pica: strip %d: ...", :110-114)
                }
#ifndef MIC_PICA_NO_PICK
                const size_t bytes = (size_t)(offs[(size_t)(2 * (e - s0))] - offs[(size_t)(2 * (q - s0))]);
                if (!r.failed() && (rc = r.dst.append(*downs.back(), s->device, d_blobs + offs[(size_t)(2 * (q - s0))], bytes))) return rc;
#else
                for (int z = q; z < e && !r.failed(); z++) {
                    const size_t a = (size_t)(2 * (z - s0)) + r.flag[(size_t)strips[(size_t)z].idx], bytes = (size_t)(offs[a + 1] - offs[a]);
                    if ((rc = r.dst.append(*downs.back(), s->device, d_blobs + offs[a], bytes))) return rc;
                }
#endif
                q = e;
            }
            s0 = s1;
        }
        return MIC_OK;
    });
    for (auto &d : downs) { const int r2 = d->wait(); if (rc == MIC_OK) rc = r2; }
    return rc;
}

// ============================================================================ strip files: PICS (parallelstrips.go), PICA (parallelstripsadaptive.go)
// The batch decoder of both: a file is a header and one unit per strip.  info: the file's width, height and strip count;
// entry(c, h, n, k): strip k as its header states it (pics_strip_entry / pica_strip_entry, mic_session.h); pica: the call is a PICA
// one (-DMIC_PICA_TIMING builds time those).
// crc (with it the call takes digests; null: not): crc[i] = the CRC-32 of job i's image, its strips' CRCs joined in order; expect
// (nullable): a decoded job whose CRC differs becomes MIC_ERR_MISMATCH.
template <class Job, class Info, class Entry>
int strips_decompress_batch(Job *jobs, int njobs, bool pica, Info info, Entry entry, const uint32_t *expect = nullptr, uint32_t *crc = nullptr) {
    if (!jobs || njobs < 0) return MIC_ERR_ARGS;
    for (int i = 0; crc && i < njobs; i++) crc[i] = 0;
    if (njobs == 0) return MIC_OK;
    int rc = ensure_device();
    if (rc) return rc;
    std::vector<DecGroup> G; std::vector<DecUnit> U; std::vector<int> job_of;
    for (int i = 0; i < njobs; i++) {
        Job &j = jobs[i];
        j.failed_strip = -1;
        if (!j.compressed || !j.pixels_out) { j.status = MIC_ERR_ARGS; continue; }
        int w, h, n;
        if ((j.status = info(j.compressed, j.compressed_len, &w, &h, &n))) continue;
        if (w != j.width || h != j.height) { j.status = MIC_ERR_ARGS; continue; }
        const size_t u0 = U.size();
        int32_t bad = MIC_OK; size_t covered = 0;
        for (int k = 0; k < n && bad == MIC_OK; k++) {
            const StripEntry e = entry(j.compressed, h, n, k);
            if ((bad = strip_entry_check(e, w, h, j.compressed_len))) break;
            U.push_back(DecUnit{ e.start, e.len, (uint64_t)e.y0 * (uint64_t)w, w, (int32_t)(e.y1 - e.y0), e.flags, (int)G.size() });
            covered += (size_t)w * (size_t)(e.y1 - e.y0);
        }
        if (bad != MIC_OK) { U.resize(u0); j.status = bad; continue; }
        // pixels no strip writes come back as zeros, like the reference's make([]uint16, w*h) (parallelstrips.go:288,
        // parallelstripsadaptive.go:175): a header whose strips do not cover the image is accepted there
        if (covered < (size_t)w * (size_t)h) memset(j.pixels_out, 0, (size_t)w * (size_t)h * 2);
        if (crc && covered != (size_t)w * (size_t)h) { U.resize(u0); j.status = MIC_ERR_UNSUPPORTED; continue; }   // (strips that leave holes or overlap: no fold of strip digests is the image's)
        G.push_back(DecGroup{ j.compressed, j.pixels_out, (int)u0, n });
        job_of.push_back(i);
    }
#ifdef MIC_PICA_TIMING
    DefaultLease lease;                                 // (the call then runs on this session: one device)
    if (pica && (rc = lease.acquire())) return rc;
    std::unique_ptr<PicaTimingScope> timing(pica ? new PicaTimingScope(lease.s, "decode") : nullptr);
#endif
    if ((rc = over_devices((int)G.size(), [&](int g) { return group_px(G[(size_t)g], U); },
                           [&](mic_hip_session *s, int g0, int g1) { return decode_groups(s, G, U, g0, g1, crc != nullptr); }))) return rc;
    for (size_t k = 0; k < G.size(); k++) { jobs[job_of[k]].status = G[k].status; jobs[job_of[k]].failed_strip = G[k].failed; }   // "strip %d: %w", parallelstrips.go:316; "pica: strip %d: %w", :207
    for (size_t k = 0; crc && k < G.size(); k++) {
        if (G[k].status != MIC_OK) continue;
        uint32_t c = 0;
        for (int q = G[k].first; q < G[k].first + G[k].n; q++) {
            const DecUnit &u = U[(size_t)q];
            c = q == G[k].first ? u.crc : mic_hip_crc32_combine(c, u.crc, 2 * (uint64_t)u.w * (uint64_t)u.h);
        }
        crc[job_of[k]] = c;
        if (expect && expect[job_of[k]] != c) jobs[job_of[k]].status = MIC_ERR_MISMATCH;
    }
    return MIC_OK;
}

// ============================================================================ RGB: many images per call (mic_rgb_batch.hip)
// The call's jobs are cut into sub-batches of whole images (rgb_next_cut: their units under the workspace ceiling, about a part's
// share of the pixels) and run on run_staged; a sub-batch's images come up back to back -- so an image starts at whatever byte its
// neighbours leave -- and its blobs, assembled on the device, go down from its half of the payload, one copy per job.
inline size_t rgb_target_px(size_t images, size_t total_px, bool encode) {
    static const char *ov = getenv("MIC_HIP_PIPELINE_PARTS");              // (as pipeline_target: force the number of parts)
    // a unit chain costs about the same for a few units as for hundreds: parts of >= 256 / 384 units (encode / decode), three / two at most
    const size_t parts = ov ? (size_t)std::max(1, atoi(ov)) : std::min<size_t>(encode ? 3 : 2, 3 * images / (encode ? 256 : 384));
    if (parts < 2) return ~(size_t)0;
    return std::max<size_t>(1, (total_px + parts - 1) / parts);
}
// jobs J[j0 .. j1) (checked: arguments fine) on session s
int rgb_encode_host(mic_hip_session *s, std::vector<mic_hip_rgb_enc_job *> &J, int j0, int j1) {
    if (j0 >= j1) return MIC_OK;
    int rc = s->ensure(1, 1);                                             // (the stream)
    if (rc) return rc;
    auto npx = [&](int i) { return (size_t)J[(size_t)i]->width * (size_t)J[(size_t)i]->height; };
    size_t total_px = 0;
    for (int i = j0; i < j1; i++) total_px += npx(i);
    const size_t target = rgb_target_px((size_t)(j1 - j0), total_px, true);
    struct Sub { int i0, i1; std::vector<RgbImage> img; size_t bytes; };
    std::vector<Sub> subs = staged_cut<Sub>(j0, j1, [&](int i0) { return rgb_next_cut(npx, i0, j1, target); }, [&](int i0, int i1) {
        Sub sb{ i0, i1, {}, 0 };
        for (int i = i0; i < i1; i++) {
            sb.img.push_back(RgbImage{ (uint64_t)sb.bytes, J[(size_t)i]->width, J[(size_t)i]->height, J[(size_t)i]->container, MIC_OK, -1, 0, 0 });
            sb.bytes += npx(i) * 3;
        }
        return sb;
    });
    for (size_t k = 0; k < subs.size(); k++) trace_part("rgb encode", k, subs.size(), "images", subs[k].i0, subs[k].i1, subs[k].bytes / 3);
    DevBuf *in[2] = { &s->io_px, &s->io_px2 }, *pay[2] = { &s->rgb_payload, &s->rgb_payload2 };
    return run_staged(subs.size(), [&](size_t k, int half, IoReq &up) -> int {
        const Sub &sb = subs[k];
        int r = in[half]->reserve(sb.bytes + 64);
        for (int i = sb.i0; i < sb.i1 && r == MIC_OK; i++)
            r = io_submit(up, s->device, (uint8_t *)in[half]->p + sb.img[(size_t)(i - sb.i0)].rgb_off, J[(size_t)i]->rgb, npx(i) * 3, true);
        return r;
    }, [&](size_t k, int half, IoReq &down, IoReq *) -> int {
        Sub &sb = subs[k];
        uint64_t end = 0;
        int rc = rgb_encode_run(s, (const uint8_t *)in[half]->p, sb.img.data(), sb.i1 - sb.i0, *pay[half], 0, &end);
        for (int i = sb.i0; i < sb.i1 && rc == MIC_OK; i++) {
            mic_hip_rgb_enc_job &j = *J[(size_t)i];
            const RgbImage &im = sb.img[(size_t)(i - sb.i0)];
            j.status = im.status; j.failed_plane = im.failed_plane;
            if (j.status != MIC_OK) continue;
            if (im.blob_len > j.out_cap) { j.status = MIC_ERR_CAPACITY; continue; }
            rc = io_submit(down, s->device, (uint8_t *)pay[half]->p + im.blob_off, j.out, (size_t)im.blob_len, false);   // the job's bytes: one copy
            j.out_len = (size_t)im.blob_len;
        }
        return rc;
    });
}

struct RgbDecRun { mic_hip_rgb_dec_job *j; const uint8_t *blob; size_t len; int32_t w, h; RgbPlaneRec pl[3]; };
int rgb_decode_host(mic_hip_session *s, std::vector<RgbDecRun> &J, int j0, int j1) {
    if (j0 >= j1) return MIC_OK;
    int rc = s->ensure(1, 1);
    if (rc) return rc;
    auto npx = [&](int i) { return (size_t)J[(size_t)i].w * (size_t)J[(size_t)i].h; };
    size_t total_px = 0;
    for (int i = j0; i < j1; i++) total_px += npx(i);
    const size_t target = rgb_target_px((size_t)(j1 - j0), total_px, false);
    // small blobs in ordinary memory are gathered on the host and go up in one copy; large or pinned ones go up from where they lie
    struct Sub { int i0, i1; std::vector<RgbBlob> bl; std::vector<uint8_t> small; size_t comp, bytes; };
    std::vector<Sub> subs = staged_cut<Sub>(j0, j1, [&](int i0) { return rgb_next_cut(npx, i0, j1, target); }, [&](int i0, int i1) {
        Sub sb{ i0, i1, {}, {}, 0, 0 };
        for (int i = i0; i < i1; i++) {
            const RgbDecRun &r = J[(size_t)i];
            sb.bl.push_back(RgbBlob{ 0, r.len, (uint64_t)sb.bytes, r.w, r.h, MIC_OK, -1, { r.pl[0], r.pl[1], r.pl[2] } });
            sb.bytes += npx(i) * 3;
        }
        return sb;
    });
    for (size_t k = 0; k < subs.size(); k++) trace_part("rgb decode", k, subs.size(), "images", subs[k].i0, subs[k].i1, subs[k].bytes / 3);
    DevBuf *in[2] = { &s->io_comp, &s->io_comp2 }, *outb[2] = { &s->io_px, &s->io_px2 };
    return run_staged(subs.size(), [&](size_t k, int half, IoReq &up) -> int {
        Sub &sb = subs[k];
        std::vector<int> direct;
        for (int i = sb.i0; i < sb.i1; i++) {
            const RgbDecRun &r = J[(size_t)i];
            if (r.len <= kInline && !host_is_pinned(r.blob)) { sb.bl[(size_t)(i - sb.i0)].blob_off = sb.small.size(); sb.small.insert(sb.small.end(), r.blob, r.blob + r.len); }
            else direct.push_back(i);
        }
        sb.comp = sb.small.size();
        for (int i : direct) { sb.bl[(size_t)(i - sb.i0)].blob_off = sb.comp; sb.comp += J[(size_t)i].len; }
        int r = in[half]->reserve(sb.comp + 64);
        if (r == MIC_OK && !sb.small.empty()) r = io_submit(up, s->device, in[half]->p, sb.small.data(), sb.small.size(), true);
        for (size_t q = 0; q < direct.size() && r == MIC_OK; q++)
            r = io_submit(up, s->device, (uint8_t *)in[half]->p + sb.bl[(size_t)(direct[q] - sb.i0)].blob_off, J[(size_t)direct[q]].blob, J[(size_t)direct[q]].len, true);
        return r;
    }, [&](size_t k, int half, IoReq &down, IoReq *) -> int {
        Sub &sb = subs[k];
        int rc = outb[half]->reserve(sb.bytes + 64);
        if (rc == MIC_OK) rc = rgb_decode_run(s, (const uint8_t *)in[half]->p, sb.bl.data(), sb.i1 - sb.i0, (uint8_t *)outb[half]->p);
        for (int i = sb.i0; i < sb.i1 && rc == MIC_OK; i++) {
            const RgbBlob &b = sb.bl[(size_t)(i - sb.i0)];
            mic_hip_rgb_dec_job &j = *J[(size_t)i].j;
            j.status = b.status; j.failed_plane = b.failed_plane;
            if (b.status == MIC_OK) rc = io_submit(down, s->device, (uint8_t *)outb[half]->p + b.rgb_off, j.rgb_out, npx(i) * 3, false);
        }
        return rc;
    });
}

// ============================================================================ WaveletV2: frames of any shapes per call (mic_wavelet.hip)
// A shard's jobs are cut into sub-batches by wv_next_cut alone -- the rule mic_hip_wavelet_v2_batch_plan states -- and the sub-batches
// are the PARTS of run_staged: one launch chain each (one more where a reduced decode sends frames round again), and
// MIC_HIP_PIPELINE_PARTS has no say here.  A part's frames lie back to back in its staging half, its streams and bands likewise.
struct WvCount {                                       // what the shards of a call add up
    std::mutex mu; uint64_t subs = 0, chains = 0, redo = 0;
    void add(uint64_t s, uint64_t c, uint64_t r) { std::lock_guard<std::mutex> lk(mu); subs += s; chains += c; redo += r; }
};
// jobs J[j0 .. j1) (checked: arguments fine) on session s
int wv_encode_host(mic_hip_session *s, std::vector<mic_hip_wv_enc_job *> &J, int j0, int j1, WvCount &count) {
    if (j0 >= j1) return MIC_OK;
    int rc = s->ensure(1, 1);                                             // (the stream)
    if (rc) return rc;
    auto npx = [&](size_t i) { return (size_t)J[i]->rows * (size_t)J[i]->cols; };
    const size_t budget = kWorkspaceBudget;
    struct Sub { int i0, i1; std::vector<WvEncFrame> fr; size_t px; };
    const std::vector<Sub> subs = staged_cut<Sub>(j0, j1, [&](int i0) { return (int)wv_next_cut(npx, (size_t)i0, (size_t)j1, budget); }, [&](int i0, int i1) {
        Sub sb{ i0, i1, {}, 0 };
        for (int i = i0; i < i1; i++) {
            sb.fr.push_back(WvEncFrame{ (uint64_t)sb.px, J[(size_t)i]->rows, J[(size_t)i]->cols, J[(size_t)i]->levels_applied });
            sb.px += npx((size_t)i);
        }
        return sb;
    });
    for (size_t k = 0; k < subs.size(); k++) trace_part("wavelet encode", k, subs.size(), "frames", subs[k].i0, subs[k].i1, subs[k].px);
    DevBuf *in[2] = { &s->io_px, &s->io_px2 };
    IoReq *prev = nullptr;                                // the download of the part before: keep_packed waits for it
    return run_staged(subs.size(), [&](size_t k, int half, IoReq &up) -> int {
        const Sub &sb = subs[k];
        int r = in[half]->reserve(sb.px * 2 + 64);
        for (int i = sb.i0; i < sb.i1 && r == MIC_OK; i++)
            r = io_submit(up, s->device, (uint16_t *)in[half]->p + sb.fr[(size_t)(i - sb.i0)].px_off, J[(size_t)i]->pixels, npx((size_t)i) * 2, true);
        return r;
    }, [&](size_t k, int half, IoReq &down, IoReq *) -> int {
        const Sub &sb = subs[k];
        const int nb = sb.i1 - sb.i0;
        std::vector<uint64_t> offs((size_t)nb + 1); std::vector<int32_t> st((size_t)nb);
        const uint8_t *d_blobs = nullptr;
        int rc = wv_encode_run(s, (const uint16_t *)in[half]->p, sb.fr.data(), nb, &d_blobs, offs.data(), st.data());
        if (rc == MIC_OK) rc = keep_packed(s, prev);
        if (rc != MIC_OK) return rc;
        prev = &down;
        count.add(1, 1, 0);
        for (int i = sb.i0; i < sb.i1 && rc == MIC_OK; i++) {
            mic_hip_wv_enc_job &j = *J[(size_t)i];
            const size_t q = (size_t)(i - sb.i0), len = (size_t)(offs[q + 1] - offs[q]);
            if ((j.status = st[q]) != MIC_OK) continue;
            if (11 + len > j.out_cap) { j.status = MIC_ERR_CAPACITY; continue; }
            wv_put_header(j.out, j.rows, j.cols, j.max_value, j.levels_applied);
            rc = io_submit(down, s->device, const_cast<uint8_t *>(d_blobs) + offs[q], j.out + 11, len, false);   // the job's stream: one copy
            j.out_len = 11 + len;
        }
        return rc;
    });
}

// jobs J[j0 .. j1) (checked: header and arguments fine, rows / cols / levels / out_rows / out_cols set) on session s
int wv_decode_host(mic_hip_session *s, std::vector<mic_hip_wv_dec_job *> &J, int j0, int j1, WvCount &count) {
    if (j0 >= j1) return MIC_OK;
    int rc = s->ensure(1, 1);
    if (rc) return rc;
    auto npx = [&](size_t i) { return (size_t)J[i]->rows * (size_t)J[i]->cols; };
    auto band = [&](size_t i) { return (size_t)J[i]->out_rows * (size_t)J[i]->out_cols; };
    const size_t budget = kWorkspaceBudget;
    // small files in ordinary memory are gathered on the host and go up in one copy; large or pinned ones go up from where they lie
    struct Sub { int i0, i1; std::vector<WvDecFrame> fr; std::vector<uint8_t> small; size_t comp, px; };
    std::vector<Sub> subs = staged_cut<Sub>(j0, j1, [&](int i0) { return (int)wv_next_cut(npx, (size_t)i0, (size_t)j1, budget); }, [&](int i0, int i1) {
        Sub sb{ i0, i1, {}, {}, 0, 0 };
        for (int i = i0; i < i1; i++) {
            const mic_hip_wv_dec_job &j = *J[(size_t)i];
            sb.fr.push_back(WvDecFrame{ 0, 0, (uint64_t)sb.px, j.rows, j.cols, j.levels, j.level });
            sb.px += band((size_t)i);
        }
        return sb;
    });
    for (size_t k = 0; k < subs.size(); k++) trace_part("wavelet decode", k, subs.size(), "frames", subs[k].i0, subs[k].i1, subs[k].px);
    DevBuf *in[2] = { &s->io_comp, &s->io_comp2 }, *outb[2] = { &s->io_px, &s->io_px2 };
    return run_staged(subs.size(), [&](size_t k, int half, IoReq &up) -> int {
        Sub &sb = subs[k];
        std::vector<int> direct;
        auto place = [&](int i, size_t at) { WvDecFrame &f = sb.fr[(size_t)(i - sb.i0)]; f.begin = at; f.end = at + (J[(size_t)i]->compressed_len - 11); };
        for (int i = sb.i0; i < sb.i1; i++) {                                // (the streams: the files without their 11-byte headers)
            const mic_hip_wv_dec_job &j = *J[(size_t)i];
            if (j.compressed_len - 11 <= kInline && !host_is_pinned(j.compressed)) { place(i, sb.small.size()); sb.small.insert(sb.small.end(), j.compressed + 11, j.compressed + j.compressed_len); }
            else direct.push_back(i);
        }
        sb.comp = sb.small.size();
        for (int i : direct) { place(i, sb.comp); sb.comp += J[(size_t)i]->compressed_len - 11; }
        int r = in[half]->reserve(sb.comp + 64);
        if (r == MIC_OK && !sb.small.empty()) r = io_submit(up, s->device, in[half]->p, sb.small.data(), sb.small.size(), true);
        for (size_t q = 0; q < direct.size() && r == MIC_OK; q++)
            r = io_submit(up, s->device, (uint8_t *)in[half]->p + sb.fr[(size_t)(direct[q] - sb.i0)].begin, J[(size_t)direct[q]]->compressed + 11,
                          J[(size_t)direct[q]]->compressed_len - 11, true);
        return r;
    }, [&](size_t k, int half, IoReq &down, IoReq *) -> int {
        Sub &sb = subs[k];
        const int nb = sb.i1 - sb.i0;
        std::vector<int32_t> st((size_t)nb); std::vector<uint64_t> sy((size_t)nb, 0);
        uint64_t redone = 0;
        int rc = outb[half]->reserve(sb.px * 2 + 64);
        if (rc == MIC_OK) rc = wv_decode_run(s, (const uint8_t *)in[half]->p, (uint16_t *)outb[half]->p, sb.fr.data(), nb, st.data(), sy.data(), &redone);
        if (rc != MIC_OK) return rc;
        count.add(1, redone ? 2 : 1, redone);
        for (int i = sb.i0; i < sb.i1 && rc == MIC_OK; i++) {
            mic_hip_wv_dec_job &j = *J[(size_t)i];
            const size_t q = (size_t)(i - sb.i0);
            j.status = st[q]; j.symbols_decoded = sy[q];
            if (j.status == MIC_OK) rc = io_submit(down, s->device, (uint16_t *)outb[half]->p + sb.fr[q].px_off, j.pixels_out, band((size_t)i) * 2, false);
        }
        return rc;
    });
}

// ============================================================================ MIC2: many volumes per call (mic_mic2_batch.hip)
// The units of a shard's volumes -- volume order, then frame order -- are cut into sub-batches by their sizes alone
// (mic2_batch_cuts), and the sub-batches are the PARTS of run_staged: the call runs exactly the chains the planner
// (mic_hip_mic2_batch_plan) counts, and MIC_HIP_PIPELINE_PARTS has no say here.  A part's frames lie back to back in its staging half.
struct Mic2Count {                                     // what the shards of a call add up
    std::mutex mu; uint64_t slabs = 0;
    void add(uint64_t n) { std::lock_guard<std::mutex> lk(mu); slabs += n; }
};
struct Mic2Run { int vol, i0, i1, f0; uint64_t off; };  // units [i0, i1) of a part (counted from its first) are frames f0 .. of volume vol; off: where frame f0 lies in the part's pixels
struct Mic2EncVol { mic_hip_mic2_enc_job *j; size_t npx; DestRun dst; std::vector<uint32_t> len; int32_t status = MIC_OK, failed = -1; };
struct Mic2DecVol {
    mic_hip_mic2_dec_job *j; Mic2Head m; size_t npx;
    int32_t status = MIC_OK, failed = -1;
    const uint16_t *d_last = nullptr;                  // where the part before left the volume's last frame so far: the next part's carry
};
struct Mic2Part { std::vector<Mic2Run> runs; int nb = 0; size_t px = 0; };
// the parts of volumes [v0, v1) with n(v) frames of npx(v) pixels; lead(v): a run that starts behind frame 0 keeps a frame's room in front of it
template <class N, class P, class L>
std::vector<Mic2Part> mic2_parts(int v0, int v1, N &&n, P &&npx, L &&lead) {
    struct Unit { int vol, frame; };
    std::vector<Unit> un; std::vector<size_t> px;
    for (int v = v0; v < v1; v++) for (int f = 0; f < n(v); f++) { un.push_back(Unit{ v, f }); px.push_back(npx(v)); }
    const std::vector<size_t> cuts = mic2_batch_cuts(px, kWorkspaceBudget);
    std::vector<Mic2Part> parts(cuts.size() - 1);
    for (size_t b = 0; b + 1 < cuts.size(); b++) {
        Mic2Part &p = parts[b];
        p.nb = (int)(cuts[b + 1] - cuts[b]);
        for (int i = 0; i < p.nb;) {
            const Unit &u = un[cuts[b] + (size_t)i];
            int e = i + 1;
            while (e < p.nb && un[cuts[b] + (size_t)e].vol == u.vol) e++;
            if (u.frame > 0 && lead(u.vol)) p.px += px[cuts[b] + (size_t)i];
            p.runs.push_back(Mic2Run{ u.vol, i, e, u.frame, (uint64_t)p.px });
            p.px += (size_t)(e - i) * px[cuts[b] + (size_t)i];
            i = e;
        }
    }
    return parts;
}

// volumes V[v0 .. v1) (arguments fine) on session s
int mic2_encode_host(mic_hip_session *s, std::vector<Mic2EncVol> &V, int v0, int v1, Mic2Count &count) {
    if (v0 >= v1) return MIC_OK;
    int rc = s->ensure(1, 1);                                             // (the stream)
    if (rc) return rc;
    // a residual needs the ORIGINAL frame before it: a part that starts inside a temporal volume uploads that frame in front
    const std::vector<Mic2Part> parts = mic2_parts(v0, v1, [&](int v) { return V[(size_t)v].j->nframes; }, [&](int v) { return V[(size_t)v].npx; },
                                                   [&](int v) { return V[(size_t)v].j->temporal != 0; });
    count.add(parts.size());
    for (size_t k = 0; k < parts.size(); k++) trace_part("mic2 encode", k, parts.size(), "units", 0, parts[k].nb, parts[k].px);
    DevBuf *in[2] = { &s->io_px, &s->io_px2 };
    IoReq *prev = nullptr;                                // the download of the part before: keep_packed waits for it
    return run_staged(parts.size(), [&](size_t k, int half, IoReq &up) -> int {
        const Mic2Part &p = parts[k];
        int r = in[half]->reserve(p.px * 2 + 64);
        for (size_t q = 0; q < p.runs.size() && r == MIC_OK; q++) {
            const Mic2Run &run = p.runs[q];
            const Mic2EncVol &v = V[(size_t)run.vol];
            const size_t lead = (run.f0 > 0 && v.j->temporal) ? 1 : 0;
            r = io_submit(up, s->device, (uint16_t *)in[half]->p + run.off - lead * v.npx, v.j->frames + ((size_t)run.f0 - lead) * v.npx,
                          ((size_t)(run.i1 - run.i0) + lead) * v.npx * 2, true);
        }
        return r;
    }, [&](size_t k, int half, IoReq &down, IoReq *) -> int {
        const Mic2Part &p = parts[k];
        std::vector<Mic2EncUnit> u((size_t)p.nb);
        for (const Mic2Run &run : p.runs) {
            const Mic2EncVol &v = V[(size_t)run.vol];
            for (int i = run.i0; i < run.i1; i++)
                u[(size_t)i] = Mic2EncUnit{ (const uint16_t *)in[half]->p + run.off + (size_t)(i - run.i0) * v.npx, v.j->width, v.j->height, v.j->max_value,
                                            (uint16_t)(v.j->temporal && run.f0 + (i - run.i0) > 0) };
        }
        std::vector<uint64_t> offs((size_t)p.nb + 1); std::vector<int32_t> st((size_t)p.nb);
        const uint8_t *d_blobs = nullptr;
        int rc = mic2_batch_encode_units(s, u.data(), p.nb, &d_blobs, offs.data(), st.data());
        if (rc == MIC_OK) rc = keep_packed(s, prev);
        if (rc != MIC_OK) return rc;
        prev = &down;
        for (const Mic2Run &run : p.runs) {               // per volume: its streams of this part, one transfer
            Mic2EncVol &v = V[(size_t)run.vol];
            for (int i = run.i0; i < run.i1; i++) {
                const int f = run.f0 + (i - run.i0);
                v.len[(size_t)f] = (uint32_t)(offs[(size_t)i + 1] - offs[(size_t)i]);
                if (st[(size_t)i] != MIC_OK && v.status == MIC_OK) { v.status = st[(size_t)i]; v.failed = f; }   // the first failing frame names the error
            }
            if (v.status != MIC_OK) continue;
            rc = v.dst.append(down, s->device, d_blobs + offs[(size_t)run.i0], (size_t)(offs[(size_t)run.i1] - offs[(size_t)run.i0]));
            if (v.dst.cap_fail) v.status = MIC_ERR_CAPACITY;
            if (rc) return rc;
        }
        return MIC_OK;
    });
}

int mic2_decode_host(mic_hip_session *s, std::vector<Mic2DecVol> &V, int v0, int v1, Mic2Count &count) {
    if (v0 >= v1) return MIC_OK;
    int rc = s->ensure(1, 1);
    if (rc) return rc;
    const std::vector<Mic2Part> parts = mic2_parts(v0, v1, [&](int v) { return V[(size_t)v].m.n; }, [&](int v) { return V[(size_t)v].npx; },
                                                   [](int) { return false; });
    count.add(parts.size());
    for (size_t k = 0; k < parts.size(); k++) trace_part("mic2 decode", k, parts.size(), "units", 0, parts[k].nb, parts[k].px);
    DevBuf *in[2] = { &s->io_comp, &s->io_comp2 }, *outb[2] = { &s->io_px, &s->io_px2 };
    auto stream_of = [&](const Mic2DecVol &v, int f, uint32_t *len) {
        *len = get_u32(v.m.table + 8 * (size_t)f + 4);
        return v.j->compressed + 20 + 8 * (size_t)v.m.n + get_u32(v.m.table + 8 * (size_t)f);
    };
    std::vector<uint64_t> begins[2];                                      // where a part's streams lie in its half
    return run_staged(parts.size(), [&](size_t k, int half, IoReq &up) -> int {
        const Mic2Part &p = parts[k];
        std::vector<uint64_t> &bg = begins[half];
        bg.assign((size_t)p.nb + 1, 0);
        std::vector<const uint8_t *> src((size_t)p.nb);
        for (const Mic2Run &run : p.runs)
            for (int i = run.i0; i < run.i1; i++) {
                uint32_t len;
                src[(size_t)i] = stream_of(V[(size_t)run.vol], run.f0 + (i - run.i0), &len);
                bg[(size_t)i + 1] = bg[(size_t)i] + len;
            }
        int r = in[half]->reserve((size_t)bg[(size_t)p.nb] + 64);
        for (int i = 0; i < p.nb && r == MIC_OK;) {                       // streams that are neighbours in a file go up in one transfer
            int e = i + 1;
            while (e < p.nb && src[(size_t)e] == src[(size_t)i] + (bg[(size_t)e] - bg[(size_t)i])) e++;
            r = io_submit(up, s->device, (uint8_t *)in[half]->p + bg[(size_t)i], src[(size_t)i], (size_t)(bg[(size_t)e] - bg[(size_t)i]), true);
            i = e;
        }
        return r;
    }, [&](size_t k, int half, IoReq &down, IoReq *) -> int {
        const Mic2Part &p = parts[k];
        const std::vector<uint64_t> &bg = begins[half];
        int rc = outb[half]->reserve(p.px * 2 + 64);
        if (rc) return rc;
        uint16_t *d_px = (uint16_t *)outb[half]->p;
        std::vector<Mic2DecUnit> u((size_t)p.nb);
        for (const Mic2Run &run : p.runs) {
            const Mic2DecVol &v = V[(size_t)run.vol];
            for (int i = run.i0; i < run.i1; i++)
                u[(size_t)i] = Mic2DecUnit{ (const uint8_t *)in[half]->p + bg[(size_t)i], (uint32_t)(bg[(size_t)i + 1] - bg[(size_t)i]), v.m.w, v.m.h,
                                            d_px + run.off + (size_t)(i - run.i0) * v.npx, (uint32_t)(v.m.temporal && run.f0 + (i - run.i0) > 0) };
        }
        std::vector<int32_t> st((size_t)p.nb);
        if ((rc = mic2_batch_decode_units(s, u.data(), p.nb, st.data()))) return rc;
        std::vector<Mic2DecSpan> spans;
        for (const Mic2Run &run : p.runs) {
            Mic2DecVol &v = V[(size_t)run.vol];
            for (int i = run.i0; i < run.i1 && v.status == MIC_OK; i++)
                if (st[(size_t)i] != MIC_OK) { v.status = st[(size_t)i]; v.failed = run.f0 + (i - run.i0); }
            // the running sum of a part that starts inside a temporal volume goes on from the frame the part before left in the other half
            if (v.m.temporal) spans.push_back(Mic2DecSpan{ v.d_last, d_px + run.off, (uint32_t)v.npx, run.i0, run.i1 - run.i0, run.f0,
                                                           v.status == MIC_OK ? INT_MAX : v.failed, 0 });
            v.d_last = d_px + run.off + (size_t)(run.i1 - run.i0 - 1) * v.npx;
        }
        if ((rc = mic2_batch_accumulate(s, spans.data(), (int)spans.size()))) return rc;
        for (const Mic2Run &run : p.runs) {
            const Mic2DecVol &v = V[(size_t)run.vol];
            if (v.status != MIC_OK) continue;
            if ((rc = io_submit(down, s->device, d_px + run.off, v.j->frames_out + (size_t)run.f0 * v.npx, (size_t)(run.i1 - run.i0) * v.npx * 2, false))) return rc;
        }
        return MIC_OK;
    });
}

}  // namespace

namespace micapi {
int host_copy(int device, void *dev, void *host, size_t bytes, bool to_device) {
    IoReq req;
    const int rc = io_submit(req, device, dev, host, bytes, to_device);
    const int r2 = req.wait();
    return rc ? rc : r2;
}
// first[k] .. first[k + 1]: the items of shard k; boundary k is where the running weight first reaches k / shards of the total
void plan_shards(const uint64_t *w, int n, int shards, int *first) {
    uint64_t total = 0;
    for (int i = 0; i < n; i++) total += w[i] ? w[i] : 1;
    first[0] = 0;
    uint64_t run = 0; int i = 0;
    for (int k = 1; k < shards; k++) {
        const uint64_t goal = (uint64_t)(((unsigned __int128)total * (unsigned)k) / (unsigned)shards);
        while (i < n && run < goal) { run += w[i] ? w[i] : 1; i++; }
        first[k] = i;
    }
    first[shards] = n;
}
int run_parallel(int n, const std::function<int(int)> &work) {
    std::vector<int> rcs((size_t)std::max(n, 0), MIC_OK);
    auto one = [&](int k) {
        try { rcs[(size_t)k] = work(k); }
        catch (...) { rcs[(size_t)k] = exception_code(); }
    };
    std::vector<std::thread> th;
    int started = 1;                                  // 1 .. started - 1 have a thread; what could not get one runs here, one after the other
    try {
        th.reserve((size_t)std::max(n, 1));
        for (; started < n; started++) th.emplace_back(one, started);
    } catch (...) { }                                 // (no exception crosses the C ABI: a thread the system refuses costs overlap, not the call)
    if (n > 0) one(0);
    for (int k = started; k < n; k++) one(k);
    for (auto &t : th) t.join();
    for (int r : rcs) if (r != MIC_OK) return r;
    return MIC_OK;
}
int over_devices(const std::vector<int> &first, const ShardWork &work) {
    const std::vector<int> devs = default_devices();
    const int cut = (int)first.size() - 1;
    if (cut < 1) return MIC_ERR_INTERNAL;
    const int shards = (cur_default() || (size_t)cut > devs.size()) ? 1 : cut;   // (a nested call runs on the session its thread already holds)
    return run_parallel(shards, [&](int k) -> int {
        const int i0 = shards == 1 ? first.front() : first[(size_t)k], i1 = shards == 1 ? first.back() : first[(size_t)k + 1];
        if (i0 >= i1) return MIC_OK;
        DefaultLease lease;
        const int rc = lease.acquire(shards == 1 ? -1 : devs[(size_t)k]);
        if (rc) return rc;
        if (io_trace()) fprintf(stderr, "[mic_hip devices] shard %d of %d on device %d: items %d .. %d\n", k + 1, shards, lease.s->device, i0, i1 - 1);
        return work(lease.s, i0, i1);
    });
}
int over_devices(int n, const std::function<uint64_t(int)> &weight, const ShardWork &work) {
    const int shards = cur_default() ? 1 : (int)std::min<size_t>(default_devices().size(), (size_t)std::max(n, 0));
    std::vector<int> first{ 0, n };
    if (shards > 1) {
        std::vector<uint64_t> w((size_t)n);
        for (int i = 0; i < n; i++) w[(size_t)i] = weight(i);
        first.resize((size_t)shards + 1);
        plan_shards(w.data(), n, shards, first.data());
    }
    return over_devices(first, work);
}
}  // namespace micapi

// ================================================================================ C ABI
extern "C" {

// The cut of `n` weighted items into `shards` contiguous shards that the batch entry points use across the devices of
// mic_hip_set_devices (first[0 .. shards]: item i belongs to shard k iff first[k] <= i < first[k + 1]); no device needed.
// crc(A || B) = crc(A) * x^(8 |B|) xor crc(B): the init and final xor of the two finished CRCs cancel (mic_verify.h)
uint32_t mic_hip_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return mic_crc_mul(crc_a, mic_crc_xpow8(len_b)) ^ crc_b; }

int mic_hip_shard_plan(const uint64_t *weights, int n, int shards, int *first) try {
    if (!weights || !first || n < 0 || shards <= 0) return MIC_ERR_ARGS;
    plan_shards(weights, n, shards, first);
    return MIC_OK;
} MIC_ABI_CATCH

// Pinned host memory for a caller's frame and stream buffers: the entry points below DMA such buffers in place instead of
// staging them through the transfer engine's slots.
void *mic_hip_host_alloc(size_t bytes) {
    if (ensure_device() != MIC_OK) return nullptr;                       // (makes the default device current; no session is held or made)
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
void mic_hip_host_free(void *p) { if (p) (void)hipHostFree(p); }

// What the verified doors report of a group: its units' results joined in order -- the CRCs by mic_hip_crc32_combine (the units are
// contiguous runs of the group's pixels), the mismatches summed, the first one as the group's pixel index.  *failed (nullable): the
// first unit that mismatched, counted from the group's first.  status: the group's codec status, or MIC_ERR_MISMATCH.
static mic_hip_verify_result group_verify_result(const EncGroup &g, const std::vector<EncUnit> &U, int *failed) {
    mic_hip_verify_result r{ g.status, 0, 0, -1 };
    for (int q = g.first; q < g.first + g.n; q++) {
        const EncUnit &u = U[(size_t)q];
        r.crc32 = q == g.first ? u.vr.crc32 : mic_hip_crc32_combine(r.crc32, u.vr.crc32, 2 * (uint64_t)u.w * (uint64_t)u.h);
        if (u.vr.mismatches && r.mismatches == 0) {
            r.first_mismatch = (int64_t)u.px_off - (int64_t)U[(size_t)g.first].px_off + u.vr.first_mismatch;
            if (failed && g.status == MIC_OK) *failed = q - g.first;
        }
        r.mismatches += u.vr.mismatches;
    }
    if (g.status == MIC_OK && r.mismatches) r.status = MIC_ERR_MISMATCH;
    if (g.status != MIC_OK) { r.mismatches = 0; r.first_mismatch = -1; }       // (the job was not delivered: what its other units said is no use)
    return r;
}

// flags: OR-ed into every unit's nstates (MIC_HIP_GAP_REMOVAL for the _gap entry points); res (nullable): the verified door
static int compress_jobs(mic_hip_enc_job *jobs, int njobs, uint16_t flags, mic_hip_verify_result *res = nullptr) {
    if (!jobs || njobs < 0) return MIC_ERR_ARGS;
    if (njobs == 0) return MIC_OK;
    int rc = ensure_device();
    if (rc) return rc;
    std::vector<EncGroup> G; std::vector<EncUnit> U; std::vector<int> job_of;
    for (int i = 0; i < njobs; i++) {
        mic_hip_enc_job &j = jobs[i];
        j.out_len = 0; j.nstates_used = 0;
        if (res) res[i] = mic_hip_verify_result{ MIC_ERR_ARGS, 0, 0, -1 };
        if (!j.pixels || !j.out || j.width <= 0 || j.height <= 0 || (size_t)j.width * (size_t)j.height > ((size_t)1 << 28) ||
            !(j.nstates == 2 || j.nstates == 4 || j.nstates == 8)) { j.status = MIC_ERR_ARGS; continue; }
        G.push_back(EncGroup{ j.pixels, DestRun{ j.out, j.out_cap, 0 }, (int)U.size(), 1 });
        U.push_back(EncUnit{ 0, j.width, j.height, j.max_value, (uint16_t)(j.nstates | flags), (int)G.size() - 1 });
        job_of.push_back(i);
    }
    if ((rc = over_devices((int)G.size(), [&](int g) { return group_px(G[(size_t)g], U); },
                           [&](mic_hip_session *s, int g0, int g1) { return encode_groups(s, G, U, g0, g1, res != nullptr); }))) return rc;
    for (size_t k = 0; k < G.size(); k++) {
        mic_hip_enc_job &j = jobs[job_of[k]];
        j.status = G[k].status; j.nstates_used = U[k].nstates_used;
        j.out_len = G[k].status == MIC_OK ? G[k].dst.written : 0;
        if (res) j.status = (res[job_of[k]] = group_verify_result(G[k], U, nullptr)).status;   // (MIC_ERR_MISMATCH: the bytes stand, out_len says how many)
    }
    return MIC_OK;
}
int mic_hip_compress_batch_verified(mic_hip_enc_job *jobs, int njobs, mic_hip_verify_result *res) try {
    if (!res && njobs > 0) return MIC_ERR_ARGS;
    return compress_jobs(jobs, njobs, 0, res);
} MIC_ABI_CATCH
int mic_hip_compress_batch(mic_hip_enc_job *jobs, int njobs) try {
    return compress_jobs(jobs, njobs, 0);
} MIC_ABI_CATCH
int mic_hip_compress_batch_gap(mic_hip_enc_job *jobs, int njobs) try {
    return compress_jobs(jobs, njobs, MIC_HIP_GAP_REMOVAL);
} MIC_ABI_CATCH

// crc (with it the call takes digests), expect (nullable): as strips_decompress_batch's
static int decompress_jobs(mic_hip_dec_job *jobs, int njobs, uint16_t flags, const uint32_t *expect = nullptr, uint32_t *crc = nullptr) {
    if (!jobs || njobs < 0) return MIC_ERR_ARGS;
    for (int i = 0; crc && i < njobs; i++) crc[i] = 0;
    if (njobs == 0) return MIC_OK;
    int rc = ensure_device();
    if (rc) return rc;
    std::vector<DecGroup> G; std::vector<DecUnit> U; std::vector<int> job_of;
    for (int i = 0; i < njobs; i++) {
        mic_hip_dec_job &j = jobs[i];
        if (!j.compressed || !j.pixels_out || j.width <= 0 || j.height <= 0 || j.compressed_len == 0 ||
            j.compressed_len > 0xFFFFFFF0ull || (size_t)j.width * (size_t)j.height > ((size_t)1 << 28)) {
            j.status = (j.compressed && j.compressed_len == 0) ? MIC_ERR_CORRUPT : MIC_ERR_ARGS; continue;
        }
        G.push_back(DecGroup{ j.compressed, j.pixels_out, (int)U.size(), 1 });
        U.push_back(DecUnit{ 0, j.compressed_len, 0, j.width, j.height, flags, (int)G.size() - 1 });
        job_of.push_back(i);
    }
    if ((rc = over_devices((int)G.size(), [&](int g) { return group_px(G[(size_t)g], U); },
                           [&](mic_hip_session *s, int g0, int g1) { return decode_groups(s, G, U, g0, g1, crc != nullptr); }))) return rc;
    for (size_t k = 0; k < G.size(); k++) {
        jobs[job_of[k]].status = G[k].status;
        if (!crc || G[k].status != MIC_OK) continue;
        crc[job_of[k]] = U[k].crc;
        if (expect && expect[job_of[k]] != U[k].crc) jobs[job_of[k]].status = MIC_ERR_MISMATCH;
    }
    return MIC_OK;
}
int mic_hip_decompress_batch_crc(mic_hip_dec_job *jobs, int njobs, const uint32_t *expect, uint32_t *crc) try {
    if (!crc && njobs > 0) return MIC_ERR_ARGS;
    return decompress_jobs(jobs, njobs, 0, expect, crc);
} MIC_ABI_CATCH
int mic_hip_decompress_batch(mic_hip_dec_job *jobs, int njobs) try {
    return decompress_jobs(jobs, njobs, 0);
} MIC_ABI_CATCH
int mic_hip_decompress_batch_gap(mic_hip_dec_job *jobs, int njobs) try {
    return decompress_jobs(jobs, njobs, MIC_HIP_GAP_REMOVAL);
} MIC_ABI_CATCH

// ---- PICS (parallelstrips.go) ----------------------------------------------------------------
// res (nullable): the verified door
static int pics_compress_jobs(mic_hip_pics_enc_job *jobs, int njobs, mic_hip_verify_result *res) {
    if (!jobs || njobs < 0) return MIC_ERR_ARGS;
    if (njobs == 0) return MIC_OK;
    int rc = ensure_device();
    if (rc) return rc;
    std::vector<EncGroup> G; std::vector<EncUnit> U; std::vector<int> job_of;
    struct Geo { int strip_h, actual; };
    std::vector<Geo> geo;
    for (int i = 0; i < njobs; i++) {
        mic_hip_pics_enc_job &j = jobs[i];
        j.out_len = 0; j.failed_strip = -1;
        if (res) res[i] = mic_hip_verify_result{ MIC_ERR_ARGS, 0, 0, -1 };
        if (!j.pixels || !j.out || j.width <= 0 || j.height <= 0 || j.num_strips <= 0 || !(j.nstates == 2 || j.nstates == 4 || j.nstates == 8)) { j.status = MIC_ERR_ARGS; continue; }
        int strip_h, actual; pics_geometry(j.height, j.num_strips, strip_h, actual);
        const size_t header = 20 + (size_t)actual * 8;
        if ((size_t)j.width * (size_t)strip_h > ((size_t)1 << 28)) { j.status = MIC_ERR_UNSUPPORTED; if (res) res[i].status = j.status; continue; }
        if (j.out_cap < header) { j.status = MIC_ERR_CAPACITY; if (res) res[i].status = j.status; continue; }
        G.push_back(EncGroup{ j.pixels, DestRun{ j.out, j.out_cap, header }, (int)U.size(), actual });
        for (int s = 0; s < actual; s++) {
            const int y0 = s * strip_h, y1 = std::min(j.height, y0 + strip_h);
            U.push_back(EncUnit{ (uint64_t)y0 * (uint64_t)j.width, j.width, y1 - y0, j.max_value, j.nstates, (int)G.size() - 1 });   // global maxValue for every strip, :88
        }
        job_of.push_back(i); geo.push_back(Geo{ strip_h, actual });
    }
    if ((rc = over_devices((int)G.size(), [&](int g) { return group_px(G[(size_t)g], U); },
                           [&](mic_hip_session *s, int g0, int g1) { return encode_groups(s, G, U, g0, g1, res != nullptr); }))) return rc;
    for (size_t k = 0; k < G.size(); k++) {
        mic_hip_pics_enc_job &j = jobs[job_of[k]];
        const EncGroup &g = G[k];
        j.status = g.status;                                                   // first failing strip, :95-99
        j.failed_strip = g.failed;                                             // "parallelstrips: strip %d: %w", :97
        if (res) res[job_of[k]] = group_verify_result(g, U, &j.failed_strip);
        if (j.status != MIC_OK) continue;
        if (g.dst.written > 0xFFFFFFFFull) { j.status = MIC_ERR_UNSUPPORTED; if (res) res[job_of[k]].status = j.status; continue; }
        if (res) j.status = res[job_of[k]].status;                             // (MIC_ERR_MISMATCH: the file is written all the same)
        uint8_t *out = j.out;
        memcpy(out, "PICS", 4);
        put_u32(out + 4, (uint32_t)j.width); put_u32(out + 8, (uint32_t)j.height);
        put_u32(out + 12, (uint32_t)geo[k].actual); put_u32(out + 16, (uint32_t)geo[k].strip_h);
        size_t off = 0;
        for (int s = 0; s < g.n; s++) {
            const size_t len = U[(size_t)(g.first + s)].len;
            put_u32(out + 20 + (size_t)s * 8, (uint32_t)off);
            put_u32(out + 24 + (size_t)s * 8, (uint32_t)len);
            off += len;
        }
        j.out_len = g.dst.hdr + g.dst.written;
    }
    return MIC_OK;
}
int mic_hip_pics_compress_batch(mic_hip_pics_enc_job *jobs, int njobs) try {
    return pics_compress_jobs(jobs, njobs, nullptr);
} MIC_ABI_CATCH
int mic_hip_pics_compress_batch_verified(mic_hip_pics_enc_job *jobs, int njobs, mic_hip_verify_result *res) try {
    if (!res && njobs > 0) return MIC_ERR_ARGS;
    return pics_compress_jobs(jobs, njobs, res);
} MIC_ABI_CATCH

int mic_hip_pics_compress(const uint16_t *pixels, int width, int height, uint16_t max_value, int num_strips, int nstates,
                          uint8_t *out, size_t out_cap, size_t *out_len) try {
    return mic_hip_pics_compress_ex(pixels, width, height, max_value, num_strips, nstates, out, out_cap, out_len, nullptr);
} MIC_ABI_CATCH
int mic_hip_pics_compress_ex(const uint16_t *pixels, int width, int height, uint16_t max_value, int num_strips, int nstates,
                             uint8_t *out, size_t out_cap, size_t *out_len, int *failed_strip) try {
    if (failed_strip) *failed_strip = -1;
    if (!pixels || !out || !out_len || width <= 0 || height <= 0 || num_strips <= 0) return MIC_ERR_ARGS;
    if (!(nstates == 2 || nstates == 4 || nstates == 8)) return MIC_ERR_ARGS;
    mic_hip_pics_enc_job j{};
    j.pixels = pixels; j.width = width; j.height = height; j.max_value = max_value; j.nstates = (uint16_t)nstates; j.num_strips = num_strips;
    j.out = out; j.out_cap = out_cap;
    const int rc = mic_hip_pics_compress_batch(&j, 1);
    if (rc) return rc;
    if (j.status == MIC_OK) *out_len = j.out_len;
    else if (failed_strip) *failed_strip = j.failed_strip;
    return j.status;
} MIC_ABI_CATCH

int mic_hip_pics_decompress_batch(mic_hip_pics_dec_job *jobs, int njobs) try {
    return strips_decompress_batch(jobs, njobs, false,
        [](const uint8_t *c, size_t len, int *w, int *h, int *n) { return mic_hip_pics_info(c, len, w, h, n, nullptr); }, pics_strip_entry);
} MIC_ABI_CATCH

int mic_hip_pics_decompress_batch_crc(mic_hip_pics_dec_job *jobs, int njobs, const uint32_t *expect, uint32_t *crc) try {
    if (!crc && njobs > 0) return MIC_ERR_ARGS;
    return strips_decompress_batch(jobs, njobs, false,
        [](const uint8_t *c, size_t len, int *w, int *h, int *n) { return mic_hip_pics_info(c, len, w, h, n, nullptr); }, pics_strip_entry, expect, crc);
} MIC_ABI_CATCH

int mic_hip_pics_decompress(const uint8_t *c, size_t len, uint16_t *pixels_out, int width, int height) try {
    return mic_hip_pics_decompress_ex(c, len, pixels_out, width, height, nullptr);
} MIC_ABI_CATCH
int mic_hip_pics_decompress_ex(const uint8_t *c, size_t len, uint16_t *pixels_out, int width, int height, int *failed_strip) try {
    if (failed_strip) *failed_strip = -1;
    if (!c || !pixels_out) return MIC_ERR_ARGS;
    mic_hip_pics_dec_job j{};
    j.compressed = c; j.compressed_len = len; j.pixels_out = pixels_out; j.width = width; j.height = height;
    const int rc = mic_hip_pics_decompress_batch(&j, 1);
    if (rc == MIC_OK && j.status != MIC_OK && failed_strip) *failed_strip = j.failed_strip;
    return rc ? rc : j.status;
} MIC_ABI_CATCH

// ---- PICA (parallelstripsadaptive.go) ----------------------------------------------------------
int mic_hip_pica_compress_batch(mic_hip_pica_enc_job *jobs, int njobs) try {
    if (!jobs || njobs < 0) return MIC_ERR_ARGS;
    if (njobs == 0) return MIC_OK;
    int rc = ensure_device();
    if (rc) return rc;
    std::vector<PicaRun> J;
    for (int i = 0; i < njobs; i++) {
        mic_hip_pica_enc_job &j = jobs[i];
        j.out_len = 0; j.failed_strip = -1;
        if (!j.pixels || !j.out || j.width <= 0 || j.height <= 0 || j.num_strips <= 0) { j.status = MIC_ERR_ARGS; continue; }
        if ((size_t)j.width * (size_t)j.height > ((size_t)1 << 31)) { j.status = MIC_ERR_UNSUPPORTED; continue; }
        PicaRun r; r.j = &j; r.n = std::min(j.num_strips, j.height);                             // :61-66
        r.dst = DestRun{ j.out, j.out_cap, 16 + 16 * (size_t)r.n };
        if (j.out_cap < r.dst.hdr) { j.status = MIC_ERR_CAPACITY; continue; }
        r.y0.assign((size_t)r.n, 0); r.err.assign((size_t)r.n, MIC_OK); r.len.assign((size_t)r.n, 0); r.flag.assign((size_t)r.n, 0);
        j.status = MIC_ERR_DEVICE;                                                                 // (until the job has run: a call that fails as a whole leaves no stale status)
        J.push_back(std::move(r));
    }
    rc = over_devices((int)J.size(), [&](int i) { return (uint64_t)J[(size_t)i].j->width * (uint64_t)J[(size_t)i].j->height; },
                      [&](mic_hip_session *s, int j0, int j1) { return pica_encode_run(s, J, j0, j1); });
    if (rc) return rc;
    for (PicaRun &r : J) {
        mic_hip_pica_enc_job &j = *r.j;
        j.status = MIC_OK;
        for (int k = 0; k < r.n && j.status == MIC_OK; k++)
            if (r.err[(size_t)k] != MIC_OK) { j.status = r.err[(size_t)k]; j.failed_strip = k; }   // the first strip, in strip order (:110-114)
        if (j.status == MIC_OK && r.dst.cap_fail) j.status = MIC_ERR_CAPACITY;
        if (j.status == MIC_OK && r.dst.written > 0xFFFFFFFFull) j.status = MIC_ERR_UNSUPPORTED;    // u32 offsets (:120-128)
        if (j.status != MIC_OK) continue;
        uint8_t *out = j.out;
        memcpy(out, "PICA", 4);
        put_u32(out + 4, (uint32_t)j.width); put_u32(out + 8, (uint32_t)j.height); put_u32(out + 12, (uint32_t)r.n);
        size_t off = 0;
        for (int k = 0; k < r.n; k++) {
            uint8_t *e = out + 16 + (size_t)k * 16;
            put_u32(e, (uint32_t)r.y0[(size_t)k]); put_u32(e + 4, (uint32_t)off); put_u32(e + 8, r.len[(size_t)k]); put_u32(e + 12, r.flag[(size_t)k]);
            off += r.len[(size_t)k];
        }
        j.out_len = r.dst.hdr + r.dst.written;
    }
    return MIC_OK;
} MIC_ABI_CATCH

// CompressParallelStripsAdaptive (parallelstripsadaptive.go:54-137): a batch of one
int mic_hip_pica_compress(const uint16_t *pixels, int width, int height, uint16_t max_value, int num_strips,
                          uint8_t *out, size_t out_cap, size_t *out_len) try {
    return mic_hip_pica_compress_ex(pixels, width, height, max_value, num_strips, out, out_cap, out_len, nullptr);
} MIC_ABI_CATCH
int mic_hip_pica_compress_ex(const uint16_t *pixels, int width, int height, uint16_t max_value, int num_strips,
                             uint8_t *out, size_t out_cap, size_t *out_len, int *failed_strip) try {
    if (failed_strip) *failed_strip = -1;
    if (!pixels || !out || !out_len || width <= 0 || height <= 0 || num_strips <= 0) return MIC_ERR_ARGS;
    mic_hip_pica_enc_job j{};
    j.pixels = pixels; j.width = width; j.height = height; j.max_value = max_value; j.num_strips = num_strips;
    j.out = out; j.out_cap = out_cap;
    const int rc = mic_hip_pica_compress_batch(&j, 1);
    if (rc) return rc;
    if (j.status == MIC_OK) *out_len = j.out_len;
    else if (failed_strip) *failed_strip = j.failed_strip;
    return j.status;
} MIC_ABI_CATCH

int mic_hip_pica_boundaries(const uint16_t *pixels, int width, int height, int num_strips, int on_host,
                            int32_t *starts, int cap, int *n_out) try {
    if (!pixels || !starts || !n_out || width <= 0 || height <= 0 || num_strips <= 0) return MIC_ERR_ARGS;
    if ((size_t)width * (size_t)height > ((size_t)1 << 31)) return MIC_ERR_UNSUPPORTED;
    const int n = std::min(num_strips, height);
    if (cap < n) return MIC_ERR_CAPACITY;
    DefaultLease lease;
    int rc = lease.acquire();
    if (rc) return rc;
    mic_hip_session *s = lease.s;
    if ((rc = s->ensure(1, 1))) return rc;
    const size_t npx = (size_t)width * (size_t)height;
    if ((rc = s->io_px.reserve(npx * 2 + 64))) return rc;
    if ((rc = host_copy(s->device, s->io_px.p, const_cast<uint16_t *>(pixels), npx * 2, true))) return rc;
    PicaPart p;
    p.rows = (n > 1 && n < height) ? (uint32_t)height : 0u; p.nstarts = (uint32_t)n; p.px = npx;
    p.tab.push_back(MicPicaImage{ 0, width, height, n, p.rows, 0, 0 });
    if ((rc = pica_bounds_enqueue(s, p, (const uint16_t *)s->io_px.p, 0))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (!on_host) memcpy(starts, pica_starts_of(s, p, 0), 4 * (size_t)n);
    else {
        // the kernel left the inclusive prefix sums of the costs: exact integers, so their differences are the costs again
        std::vector<unsigned long long> cost((size_t)height, 0ull);
        if (p.rows) {
            HIP_TRY(hipMemcpy(cost.data(), s->pica_cost.p, 8 * (size_t)height, hipMemcpyDeviceToHost));
            for (int y = height - 1; y > 0; y--) cost[(size_t)y] -= cost[(size_t)y - 1];
        }
        const std::vector<int> ref = pica_boundaries(cost, height, n);
        if ((int)ref.size() != n) return MIC_ERR_INTERNAL;
        for (int i = 0; i < n; i++) starts[i] = ref[(size_t)i];
    }
    *n_out = n;
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_pica_decompress_batch(mic_hip_pica_dec_job *jobs, int njobs) try {
    return strips_decompress_batch(jobs, njobs, true, mic_hip_pica_info, pica_strip_entry);
} MIC_ABI_CATCH

// DecompressParallelStripsAdaptive (parallelstripsadaptive.go:141-214): a batch of one
int mic_hip_pica_decompress(const uint8_t *c, size_t len, uint16_t *pixels_out, int width, int height) try {
    return mic_hip_pica_decompress_ex(c, len, pixels_out, width, height, nullptr);
} MIC_ABI_CATCH
int mic_hip_pica_decompress_ex(const uint8_t *c, size_t len, uint16_t *pixels_out, int width, int height, int *failed_strip) try {
    if (failed_strip) *failed_strip = -1;
    if (!c || !pixels_out) return MIC_ERR_ARGS;
    mic_hip_pica_dec_job j{};
    j.compressed = c; j.compressed_len = len; j.pixels_out = pixels_out; j.width = width; j.height = height;
    const int rc = mic_hip_pica_decompress_batch(&j, 1);
    if (rc == MIC_OK && j.status != MIC_OK && failed_strip) *failed_strip = j.failed_strip;
    return rc ? rc : j.status;
} MIC_ABI_CATCH

// ---- MIC2 independent mode (multiframe.go, multiframecompress.go:179-261) -----------------------
int mic_hip_mic2_compress(const uint16_t *frames, int width, int height, int nframes, uint16_t max_value,
                          uint8_t *out, size_t out_cap, size_t *out_len) try {
    if (!frames || !out || !out_len || width <= 0 || height <= 0 || nframes <= 0) return MIC_ERR_ARGS;
    const size_t npx = (size_t)width * (size_t)height;
    if (npx > ((size_t)1 << 28)) return MIC_ERR_UNSUPPORTED;
    const size_t header = 20 + (size_t)nframes * 8;
    if (out_cap < header) return MIC_ERR_CAPACITY;
    int rc = ensure_device();
    if (rc) return rc;
    // One group per device: a shard's streams land at a provisional place of the caller's buffer -- where they would start if every
    // frame before them came out at its bound -- and are moved down behind the shard before once all lengths are known (the frames of
    // the first shard lie where they belong at once).  That needs the buffer the capacity contract promises; a smaller one: one shard.
    const size_t fb = MIC_HIP_FRAME_BOUND(npx);
    int shards = cur_default() ? 1 : (int)std::min<size_t>(default_devices().size(), (size_t)nframes / 8);
    if (shards < 1 || out_cap < header + (size_t)nframes * fb) shards = 1;
    std::vector<EncGroup> G; std::vector<EncUnit> U; std::vector<int> first(1, 0);
    for (int k = 0; k < shards; k++) {
        const int f0 = first.back(), f1 = (int)((int64_t)nframes * (k + 1) / shards);
        const size_t start = shards == 1 ? header : header + (size_t)f0 * fb;
        G.push_back(EncGroup{ frames, DestRun{ out, shards == 1 ? out_cap : start + (size_t)(f1 - f0) * fb, start }, f0, f1 - f0 });
        for (int i = f0; i < f1; i++) U.push_back(EncUnit{ (uint64_t)npx * (uint64_t)i, width, height, max_value, 2, k });
        first.push_back(f1);
    }
    // (the cut is this function's own: frames [first[k], first[k + 1]) are group k, on the k-th listed device)
    if ((rc = over_devices(first, [&](mic_hip_session *s, int f0, int f1) { return encode_groups(s, G, U, U[(size_t)f0].group, U[(size_t)f1 - 1].group + 1); }))) return rc;
    size_t written = 0;
    for (int k = 0; k < shards; k++) {
        if (G[(size_t)k].status != MIC_OK) return G[(size_t)k].status;
        if (k && G[(size_t)k].dst.written) memmove(out + header + written, out + G[(size_t)k].dst.hdr, G[(size_t)k].dst.written);
        written += G[(size_t)k].dst.written;
    }
    if (written > 0xFFFFFFFFull) return MIC_ERR_UNSUPPORTED;            // u32 offsets, multiframe.go:75-80
    memset(out, 0, 20);
    memcpy(out, "MIC2", 4);
    put_u32(out + 4, (uint32_t)width); put_u32(out + 8, (uint32_t)height); put_u32(out + 12, (uint32_t)nframes);
    out[16] = 0x01;                                                     // PipelineSpatial, multiframe.go:28
    size_t off = 0;
    for (int i = 0; i < nframes; i++) {
        put_u32(out + 20 + (size_t)i * 8, (uint32_t)off);
        put_u32(out + 24 + (size_t)i * 8, (uint32_t)U[(size_t)i].len);
        off += U[(size_t)i].len;
    }
    *out_len = header + written;
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_mic2_decompress(const uint8_t *c, size_t len, uint16_t *frames_out, size_t frames_cap_px) try {
    if (!c || !frames_out) return MIC_ERR_ARGS;
    int w, h, n, temporal;
    int rc = mic_hip_mic2_info(c, len, &w, &h, &n, &temporal);
    if (rc) return rc;
    if (w <= 0 || h <= 0 || n <= 0) return MIC_ERR_CORRUPT;
    const size_t npx = (size_t)w * (size_t)h;
    if (npx * (size_t)n > frames_cap_px) return MIC_ERR_CAPACITY;
    if (npx > ((size_t)1 << 28)) return MIC_ERR_UNSUPPORTED;
    if (temporal) return mic2_temporal_decompress(c, len, w, h, n, n, frames_out);   // mic_mic2_batch.hip
    const size_t data_off = 20 + (size_t)n * 8;
    if ((rc = ensure_device())) return rc;
    const int shards = cur_default() ? 1 : std::max(1, (int)std::min<size_t>(default_devices().size(), (size_t)n / 8));   // (frames decode into fixed places: any cut will do)
    std::vector<DecGroup> G; std::vector<DecUnit> U; std::vector<int> first(1, 0);
    for (int k = 0; k < shards; k++) {
        const int f0 = first.back(), f1 = (int)((int64_t)n * (k + 1) / shards);
        first.push_back(f1);
        G.push_back(DecGroup{ c, frames_out, f0, f1 - f0 });
        for (int i = f0; i < f1; i++) {
            const size_t start = data_off + get_u32(c + 20 + (size_t)i * 8), bl = get_u32(c + 24 + (size_t)i * 8);
            if (start + bl > len) return MIC_ERR_CORRUPT;                 // multiframe.go:137-139
            if (bl == 0) return MIC_ERR_CORRUPT;
            U.push_back(DecUnit{ start, bl, (uint64_t)npx * (uint64_t)i, w, h, 0, k });
        }
    }
    if ((rc = over_devices(first, [&](mic_hip_session *s, int f0, int f1) { return decode_groups(s, G, U, U[(size_t)f0].group, U[(size_t)f1 - 1].group + 1); }))) return rc;
    for (const DecGroup &g : G) if (g.status != MIC_OK) return g.status;
    return MIC_OK;
} MIC_ABI_CATCH

// ---- MIC2: many volumes per call, both pipelines (mic_mic2_batch.hip) ---------------------------------
int mic_hip_mic2_compress_batch(mic_hip_mic2_enc_job *jobs, int njobs, mic_hip_mic2_batch_stats *stats) try {
    if (!jobs || njobs < 0) return MIC_ERR_ARGS;
    if (stats) *stats = mic_hip_mic2_batch_stats{ 0, 0, 0 };
    if (njobs == 0) return MIC_OK;
    std::vector<Mic2EncVol> V;
    uint64_t units = 0;
    for (int i = 0; i < njobs; i++) {
        mic_hip_mic2_enc_job &j = jobs[i];
        j.out_len = 0; j.status = MIC_OK; j.failed_frame = -1;
        if (!j.frames || !j.out || j.width <= 0 || j.height <= 0 || j.nframes <= 0 || j.temporal > 1) { j.status = MIC_ERR_ARGS; continue; }
        const size_t npx = (size_t)j.width * (size_t)j.height, header = 20 + (size_t)j.nframes * 8;
        if (npx > ((size_t)1 << 28)) { j.status = MIC_ERR_UNSUPPORTED; continue; }
        if (j.out_cap < header) { j.status = MIC_ERR_CAPACITY; continue; }
        V.push_back(Mic2EncVol{ &j, npx, DestRun{ j.out, j.out_cap, header }, std::vector<uint32_t>((size_t)j.nframes, 0) });
        units += (uint64_t)j.nframes;
    }
    if (V.empty()) return MIC_OK;
    int rc = ensure_device();
    if (rc) return rc;
    Mic2Count count;
    if ((rc = over_devices((int)V.size(), [&](int v) { return (uint64_t)V[(size_t)v].npx * (uint64_t)V[(size_t)v].j->nframes; },
                           [&](mic_hip_session *s, int v0, int v1) { return mic2_encode_host(s, V, v0, v1, count); }))) return rc;
    uint64_t done = 0;
    for (Mic2EncVol &v : V) {
        mic_hip_mic2_enc_job &j = *v.j;
        if (v.status == MIC_OK && v.dst.written > 0xFFFFFFFFull) v.status = MIC_ERR_UNSUPPORTED;   // u32 offsets, multiframe.go:75-80
        j.status = v.status; j.failed_frame = v.failed;
        if (v.status != MIC_OK) continue;
        mic2_write_head(j.out, j.width, j.height, j.nframes, j.temporal != 0, v.len.data());
        j.out_len = v.dst.hdr + v.dst.written;
        done++;
    }
    if (stats) *stats = mic_hip_mic2_batch_stats{ units, count.slabs, done };
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_mic2_decompress_batch(mic_hip_mic2_dec_job *jobs, int njobs, mic_hip_mic2_batch_stats *stats) try {
    if (!jobs || njobs < 0) return MIC_ERR_ARGS;
    if (stats) *stats = mic_hip_mic2_batch_stats{ 0, 0, 0 };
    if (njobs == 0) return MIC_OK;
    std::vector<Mic2DecVol> V;
    uint64_t units = 0;
    for (int i = 0; i < njobs; i++) {
        mic_hip_mic2_dec_job &j = jobs[i];
        j.width = j.height = j.nframes = j.temporal = 0; j.status = MIC_OK; j.failed_frame = -1;
        if (!j.compressed || !j.frames_out) { j.status = MIC_ERR_ARGS; continue; }
        Mic2Head m;
        if (mic_hip_mic2_info(j.compressed, j.compressed_len, &m.w, &m.h, &m.n, &m.temporal) == MIC_OK) { j.width = m.w; j.height = m.h; j.nframes = m.n; j.temporal = m.temporal; }
        if ((j.status = mic2_batch_parse(j.compressed, j.compressed_len, j.compressed_len, m)) != MIC_OK) continue;
        const size_t npx = (size_t)m.w * (size_t)m.h;
        if (npx * (size_t)m.n > j.frames_cap_px) { j.status = MIC_ERR_CAPACITY; continue; }
        for (int f = 0; f < m.n && j.status == MIC_OK; f++) {                // multiframe.go:137-139
            const uint64_t off = 20 + 8 * (uint64_t)m.n + get_u32(m.table + 8 * (size_t)f), bl = get_u32(m.table + 8 * (size_t)f + 4);
            if (bl == 0 || off + bl > m.file_len) { j.status = MIC_ERR_CORRUPT; j.failed_frame = f; }
        }
        if (j.status != MIC_OK) continue;
        Mic2DecVol v; v.j = &j; v.m = m; v.npx = npx;
        V.push_back(v);
        units += (uint64_t)m.n;
    }
    if (V.empty()) return MIC_OK;
    int rc = ensure_device();
    if (rc) return rc;
    Mic2Count count;
    if ((rc = over_devices((int)V.size(), [&](int v) { return (uint64_t)V[(size_t)v].npx * (uint64_t)V[(size_t)v].m.n; },
                           [&](mic_hip_session *s, int v0, int v1) { return mic2_decode_host(s, V, v0, v1, count); }))) return rc;
    uint64_t done = 0;
    for (const Mic2DecVol &v : V) { v.j->status = v.status; v.j->failed_frame = v.failed; done += v.status == MIC_OK; }
    if (stats) *stats = mic_hip_mic2_batch_stats{ units, count.slabs, done };
    return MIC_OK;
} MIC_ABI_CATCH

// ---- WaveletV2 (waveletfsecompressu16.go:303-534): frames of any shapes and level counts per call ----------------------------------
int mic_hip_wavelet_v2_compress_jobs(mic_hip_wv_enc_job *jobs, int njobs, mic_hip_wv_batch_stats *stats) try {
    if (stats) *stats = mic_hip_wv_batch_stats{ 0, 0, 0, 0 };
    if (!jobs || njobs < 0) return MIC_ERR_ARGS;
    if (njobs == 0) return MIC_OK;
    std::vector<mic_hip_wv_enc_job *> J;
    for (int i = 0; i < njobs; i++) {
        mic_hip_wv_enc_job &j = jobs[i];
        j.out_len = 0; j.levels_applied = 0;
        if (!j.pixels || !j.out) { j.status = MIC_ERR_ARGS; continue; }
        if ((j.status = wv_check_shape(j.rows, j.cols))) continue;
        if (j.out_cap < 11) { j.status = MIC_ERR_CAPACITY; continue; }
        j.levels_applied = wv_levels_applied(j.rows, j.cols, j.levels);
        j.status = MIC_ERR_DEVICE;                                                                 // (until the job has run: a call that fails as a whole leaves no stale status)
        J.push_back(&j);
    }
    if (J.empty()) return MIC_OK;
    int rc = ensure_device();
    if (rc) return rc;
    WvCount count;
    if ((rc = over_devices((int)J.size(), [&](int i) { return (uint64_t)J[(size_t)i]->rows * (uint64_t)J[(size_t)i]->cols; },
                           [&](mic_hip_session *s, int j0, int j1) { return wv_encode_host(s, J, j0, j1, count); }))) return rc;
    uint64_t done = 0;
    for (int i = 0; i < njobs; i++) done += jobs[i].status == MIC_OK;
    if (stats) *stats = mic_hip_wv_batch_stats{ count.subs, count.chains, done, count.redo };
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_wavelet_v2_decompress_jobs(mic_hip_wv_dec_job *jobs, int njobs, mic_hip_wv_batch_stats *stats) try {
    if (stats) *stats = mic_hip_wv_batch_stats{ 0, 0, 0, 0 };
    if (!jobs || njobs < 0) return MIC_ERR_ARGS;
    if (njobs == 0) return MIC_OK;
    std::vector<mic_hip_wv_dec_job *> J;
    for (int i = 0; i < njobs; i++) {
        mic_hip_wv_dec_job &j = jobs[i];
        j.rows = j.cols = j.levels = j.out_rows = j.out_cols = 0; j.symbols_decoded = 0;
        if (!j.compressed || !j.pixels_out) { j.status = MIC_ERR_ARGS; continue; }
        int rows = 0, cols = 0, levels = 0;
        if ((j.status = mic_hip_wavelet_v2_info(j.compressed, j.compressed_len, &rows, &cols, nullptr, &levels))) continue;   // :494-496
        if (rows <= 0 || cols <= 0 || levels > 8) { j.status = MIC_ERR_CORRUPT; continue; }
        if ((j.status = wv_check_shape(rows, cols, levels, j.level))) continue;
        j.rows = rows; j.cols = cols; j.levels = levels;
        if ((j.status = mic_hip_wavelet_v2_level_info(j.compressed, j.compressed_len, j.level, &j.out_rows, &j.out_cols))) continue;
        if ((size_t)j.out_rows * (size_t)j.out_cols > j.out_cap_px) { j.status = MIC_ERR_CAPACITY; continue; }
        if (j.compressed_len < 13 || j.compressed[11] != 0xFF || j.compressed[12] != 0x04 || j.compressed_len - 11 > 0xFFFFFFF0ull) { j.status = MIC_ERR_CORRUPT; continue; }   // FSEDecompressU16FourState only, :503
        j.status = MIC_ERR_DEVICE;
        J.push_back(&j);
    }
    if (J.empty()) return MIC_OK;
    int rc = ensure_device();
    if (rc) return rc;
    WvCount count;
    if ((rc = over_devices((int)J.size(), [&](int i) { return (uint64_t)J[(size_t)i]->rows * (uint64_t)J[(size_t)i]->cols; },
                           [&](mic_hip_session *s, int j0, int j1) { return wv_decode_host(s, J, j0, j1, count); }))) return rc;
    uint64_t done = 0;
    for (int i = 0; i < njobs; i++) done += jobs[i].status == MIC_OK;
    if (stats) *stats = mic_hip_wv_batch_stats{ count.subs, count.chains, done, count.redo };
    return MIC_OK;
} MIC_ABI_CATCH

int mic_hip_wavelet_v2_batch_plan(const int32_t *rc, int nframes, size_t budget_bytes, uint32_t *cuts, size_t cap, uint64_t *ncuts) try {
    if (nframes < 0 || (nframes > 0 && !rc) || (cap > 0 && !cuts)) return MIC_ERR_ARGS;
    std::vector<size_t> px((size_t)nframes);
    for (int i = 0; i < nframes; i++) {
        const int32_t r = rc[2 * (size_t)i], c = rc[2 * (size_t)i + 1];
        if (r <= 0 || c <= 0) return MIC_ERR_ARGS;
        px[(size_t)i] = (size_t)r * (size_t)c;
    }
    const size_t budget = budget_bytes ? budget_bytes : kWorkspaceBudget;
    if (!budget_bytes) (void)hipGetLastError();                                             // (the default ceiling asks the device when there is one)
    std::vector<uint32_t> c{ 0 };
    while (c.back() < (uint32_t)nframes) c.push_back((uint32_t)wv_next_cut([&](size_t i) { return px[i]; }, c.back(), (size_t)nframes, budget));
    if (ncuts) *ncuts = c.size();
    if (c.size() > cap) return MIC_ERR_CAPACITY;
    std::copy(c.begin(), c.end(), cuts);
    return MIC_OK;
} MIC_ABI_CATCH

// ---- RGB (rgbcompress.go:25-33): many images per call ----------------------------------------------
int mic_hip_rgb_compress_batch(mic_hip_rgb_enc_job *jobs, int njobs) try {
    if (!jobs || njobs < 0) return MIC_ERR_ARGS;
    if (njobs == 0) return MIC_OK;
    int rc = ensure_device();
    if (rc) return rc;
    std::vector<mic_hip_rgb_enc_job *> J;
    for (int i = 0; i < njobs; i++) {
        mic_hip_rgb_enc_job &j = jobs[i];
        j.out_len = 0; j.failed_plane = -1;
        if (!j.rgb || !j.out || j.width <= 0 || j.height <= 0 || (j.container != 0 && j.container != 1)) { j.status = MIC_ERR_ARGS; continue; }
        if ((size_t)j.width * (size_t)j.height > ((size_t)1 << 26)) { j.status = MIC_ERR_UNSUPPORTED; continue; }   // as mic_hip_rgb_compress
        if (j.out_cap < (j.container ? 24u : 12u)) { j.status = MIC_ERR_CAPACITY; continue; }
        j.status = MIC_ERR_DEVICE;                                                                 // (until the job has run: a call that fails as a whole leaves no stale status)
        J.push_back(&j);
    }
    return over_devices((int)J.size(), [&](int i) { return (uint64_t)J[(size_t)i]->width * (uint64_t)J[(size_t)i]->height; },
                        [&](mic_hip_session *s, int j0, int j1) { return rgb_encode_host(s, J, j0, j1); });
} MIC_ABI_CATCH

int mic_hip_rgb_decompress_batch(mic_hip_rgb_dec_job *jobs, int njobs) try {
    if (!jobs || njobs < 0) return MIC_ERR_ARGS;
    if (njobs == 0) return MIC_OK;
    int rc = ensure_device();
    if (rc) return rc;
    std::vector<RgbDecRun> J;
    for (int i = 0; i < njobs; i++) {
        mic_hip_rgb_dec_job &j = jobs[i];
        j.failed_plane = -1;
        if (!j.compressed || !j.rgb_out || j.width < 0 || j.height < 0 || (j.container != 0 && j.container != 1)) { j.status = MIC_ERR_ARGS; continue; }
        RgbDecRun r{ &j, j.compressed, j.compressed_len, j.width, j.height, {} };
        if (j.container) {                                                                         // readMICRFile: the header names the size
            int w = 0, h = 0;
            if ((j.status = mic_hip_micr_info(j.compressed, j.compressed_len, &w, &h))) continue;
            if ((j.width || j.height) && (j.width != w || j.height != h)) { j.status = MIC_ERR_ARGS; continue; }
            r.blob += 12; r.len -= 12; r.w = w; r.h = h;
        } else if (j.width == 0 || j.height == 0) { j.status = MIC_ERR_ARGS; continue; }
        if ((size_t)r.w * (size_t)r.h > ((size_t)1 << 26)) { j.status = MIC_ERR_UNSUPPORTED; continue; }   // as mic_hip_rgb_decompress
        if ((size_t)r.w * (size_t)r.h * 3 > j.out_cap) { j.status = MIC_ERR_CAPACITY; continue; }
        RgbHead head;
        rgb_head_of(r.blob, r.len, head);
        if ((j.status = rgb_parse_head(head, r.len, (size_t)r.w * (size_t)r.h, r.pl, &j.failed_plane))) continue;
        j.status = MIC_ERR_DEVICE;
        J.push_back(r);
    }
    return over_devices((int)J.size(), [&](int i) { return (uint64_t)J[(size_t)i].w * (uint64_t)J[(size_t)i].h; },
                        [&](mic_hip_session *s, int j0, int j1) { return rgb_decode_host(s, J, j0, j1); });
} MIC_ABI_CATCH

// debug probe (not in the public header; no device): next_sub_batch over n items of px[i] pixels under a rule the caller states.  The
// capacity is a step function of the largest item, units / per items: row k of tab is (px, units), the first row whose px >= the largest
// item holds, the last row beyond it; from the first item with flag[i] != 0 (flag may be NULL) on, tab_flag's.  -> cuts [0, ..., n].
int mic_hip_debug_cuts(const uint64_t *px, const uint8_t *flag, int n, const uint64_t *tab, int ntab, const uint64_t *tab_flag, int ntab_flag,
                       uint64_t per, uint64_t limit, uint64_t item_target, uint64_t px_target, uint64_t *cuts, size_t cap, uint64_t *ncuts) try {
    if (n < 0 || (n > 0 && !px) || !tab || ntab < 1 || (flag && (!tab_flag || ntab_flag < 1)) || per < 1 || !ncuts || (cap > 0 && !cuts)) return MIC_ERR_ARGS;
    std::vector<uint64_t> c{ 0 };
    while (c.back() < (uint64_t)n) {
        bool flagged = false;
        c.push_back(next_sub_batch((size_t)c.back(), (size_t)n, [&](size_t i) { return (size_t)px[i]; }, [&](size_t i, size_t mp) {
            flagged |= flag && flag[i];
            const uint64_t *t = flagged ? tab_flag : tab;
            int k = 0;
            while (k + 1 < (flagged ? ntab_flag : ntab) && t[2 * k] < mp) k++;
            return (size_t)(t[2 * k + 1] / per);
        }, CutRule{ (size_t)limit, (size_t)item_target, (size_t)px_target }));
    }
    *ncuts = c.size();
    if (c.size() <= cap) std::copy(c.begin(), c.end(), cuts);
    return c.size() <= cap ? MIC_OK : MIC_ERR_CAPACITY;
} MIC_ABI_CATCH

}  // extern "C"
