// mic_staged.h -- the one staging pipeline of the host batch entry points (mic_host_io.hip); next_sub_batch, the one cut of a unit list.  Standard C++ only: no HIP here.
//
// A call's items are cut into PARTS.  Part k + 1 comes up into one half of the staging while part k is coded out of the other
// half and part k - 1 goes down; half = k & 1 for inputs and outputs alike.  run_staged(n, upload, run) keeps this protocol:
//   * upload(0, 0, up[0]) goes first.
//   * for k = 0 .. n - 1, in this order:
//       1. wait for up[k];
//       2. if there is a part k + 1: upload(k + 1, (k + 1) & 1, up[k + 1]) -- that half was the input of part k - 1, whose run
//          has returned;
//       3. wait for down[k - 2], if there is one -- part k writes the output half that k - 2 is (was) going down from;
//       4. run(k, k & 1, down[k], &up[k + 1] or null).  run returns with the part's kernels complete and its downloads queued
//          on down[k]; it may wait for *next_up itself to queue device work on the next part behind its own.
//   * after the first code that is not MIC_OK, from a callback or from a transfer, neither upload nor run is called again.
//   * whatever happened, every up and down has been waited for before run_staged returns: no worker thread still writes into a
//     request or into a caller's buffer.  It returns the first failure in the order above.
//   * the requests live on the heap and do not move: the transfer workers hold pointers to them.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/mic_hip.h"

struct IoReq {                                    // a set of transfers the caller waits for together
    std::atomic<int> pending{0};
    std::atomic<int> error{0};
    std::mutex mu; std::condition_variable cv;
    void add(int n) { std::lock_guard<std::mutex> lk(mu); pending.fetch_add(n); }
    void done(bool ok) {                              // (the count goes down under the lock: the waiter may free the request right after)
        std::lock_guard<std::mutex> lk(mu);
        if (!ok) error.store(1);
        if (pending.fetch_sub(1) == 1) cv.notify_all();
    }
    int wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return pending.load() == 0; });
        return error.load() ? MIC_ERR_DEVICE : MIC_OK;
    }
};

struct StagedPart { IoReq up, down; };            // a part's transfers: its input coming up, its results going down

template <class Upload, class Run>
int run_staged(size_t nparts, Upload &&upload, Run &&run) {
    std::vector<std::unique_ptr<StagedPart>> parts(nparts);
    for (auto &p : parts) p = std::make_unique<StagedPart>();
    int rc = nparts ? upload((size_t)0, 0, parts[0]->up) : MIC_OK;
    for (size_t k = 0; k < nparts && rc == MIC_OK; k++) {
        const int half = (int)(k & 1);
        rc = parts[k]->up.wait();
        if (rc == MIC_OK && k + 1 < nparts) rc = upload(k + 1, half ^ 1, parts[k + 1]->up);
        if (k >= 2) { const int r2 = parts[k - 2]->down.wait(); if (rc == MIC_OK) rc = r2; }
        if (rc == MIC_OK) rc = run(k, half, parts[k]->down, k + 1 < nparts ? &parts[k + 1]->up : nullptr);
    }
    for (auto &p : parts) { const int r2 = p->up.wait(), r3 = p->down.wait(); if (rc == MIC_OK) rc = r2 ? r2 : r3; }
    return rc;
}

// the parts of items [i0, n): next(i0) is where the part that starts at i0 ends; make(i0, i1) is the caller's record of it
template <class Part, class Next, class Make>
std::vector<Part> staged_cut(int i0, int n, Next &&next, Make &&make) {
    std::vector<Part> parts;
    while (i0 < n) { const int i1 = next(i0); parts.push_back(make(i0, i1)); i0 = i1; }
    return parts;
}

// THE greedy cut of a list of items into sub-batches: items [i0, return) of the next sub-batch of items [.., n), px(i) pixels each.
// An item joins while the count with it stays within cap(i, mp) -- the items a sub-batch may hold once item i has joined, mp the
// largest so far, i included; it is asked for every item in order and may keep running maxima of its own -- and while the items taken
// stay below `limit` (what one launch takes) and `item_target`, and their pixels below `px_target`.  The first item always joins.
struct CutRule { size_t limit, item_target = ~(size_t)0, px_target = ~(size_t)0; };
template <class Px, class Cap>                        // (a caller whose items are k units each passes capacity / k and limit / k)
size_t next_sub_batch(size_t i0, size_t n, Px &&px, Cap &&cap, const CutRule &rule) {
    size_t i1 = i0, mp = 0, sum = 0;
    while (i1 < n) {
        const size_t p = px(i1), cnt = i1 - i0;
        mp = std::max(mp, p);
        const size_t c = cap(i1, mp);
        if (cnt > 0 && (cnt + 1 > c || cnt >= rule.limit || cnt >= rule.item_target || sum >= rule.px_target)) break;
        sum += p; i1++;
    }
    return i1;
}
// cap(i, mp) of a capacity that depends on the largest item alone: f(mp), asked again only when mp has changed (f may ask the device)
template <class F>
auto cap_by_largest(F f) {
    return [f, last = ~(size_t)0, c = (size_t)0](size_t, size_t mp) mutable { if (mp != last) { last = mp; c = f(mp); } return c; };
}

// MIC_HIP_TRACE=1: the pipeline's parts, the decode's stages with wall times and the devices' shards on stderr
inline bool io_trace() { static const bool on = getenv("MIC_HIP_TRACE") != nullptr; return on; }
// "[mic_hip <what>] part k of n: <items> a .. b, <px> pixels" for part k (counted from 0) of items [i0, i1)
inline void trace_part(const char *what, size_t k, size_t n, const char *items, int i0, int i1, size_t px) {
    if (io_trace()) fprintf(stderr, "[mic_hip %s] part %zu of %zu: %s %d .. %d, %zu pixels\n", what, k + 1, n, items, i0, i1 - 1, px);
}
