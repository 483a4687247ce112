// The staging driver of the host batch entry points (csrc/mic_staged.h) on its own: no HIP, no device.  Transfers are faked with
// real IoReqs -- add(1), and a helper thread calls done(ok) a little later -- and every callback checks the protocol the header states.
//   driver <parts> <what> <k>     what: none | upload | run (the callback of part k returns an error) | up | down (a transfer of part k fails)
// Prints "ok" and exits 0, or says what broke and exits 1.
#include "mic_staged.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>

namespace {

constexpr int kUploadErr = MIC_ERR_ARGS, kRunErr = MIC_ERR_CAPACITY;   // (two codes no transfer gives: whose failure came back shows)

int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "line %d: %s: ", __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); g_bad++; } } while (0)

std::vector<std::thread> g_helpers;
std::atomic<int> g_completed{0};
int g_submitted = 0;
void fake_transfer(IoReq &r, bool ok, int ms) {
    r.add(1); g_submitted++;
    g_helpers.emplace_back([&r, ok, ms] {
        std::this_thread::sleep_for(std::chrono::milliseconds(ms));
        g_completed.fetch_add(1);                  // (before done(): once every request has pending == 0, every transfer has counted)
        r.done(ok);
    });
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: driver <parts> none|upload|run|up|down <k>\n"); return 2; }
    const size_t n = (size_t)atoi(argv[1]);
    const std::string what = argv[2];
    const size_t fk = (size_t)atoi(argv[3]);
    std::vector<IoReq *> ups(n, nullptr), downs(n, nullptr);
    size_t uploads = 0, runs_started = 0, runs_returned = 0;
    bool failed = false;                            // a callback has returned an error: nothing may be called after it

    const int rc = run_staged(n, [&](size_t k, int half, IoReq &up) -> int {
        CHECK(!failed, "upload(%zu) after a failure", k);
        CHECK(k == uploads && k < n, "upload(%zu) is call %zu", k, uploads);
        CHECK(half == (int)(k & 1), "upload(%zu) into half %d", k, half);
        // upload(k) lies between the return of run(k - 2) and the start of run(k - 1)
        const size_t before = k ? k - 1 : 0;
        CHECK(runs_started == before && runs_returned == before, "upload(%zu) with %zu runs started, %zu returned", k, runs_started, runs_returned);
        uploads++;
        if (k < n) ups[k] = &up;
        fake_transfer(up, !(what == "up" && k == fk), 3);
        fake_transfer(up, true, 1);
        if (what == "upload" && k == fk) { failed = true; return kUploadErr; }
        return MIC_OK;
    }, [&](size_t k, int half, IoReq &down, IoReq *next_up) -> int {
        CHECK(!failed, "run(%zu) after a failure", k);
        CHECK(k == runs_started && k == runs_returned && k < n, "run(%zu) with %zu runs started, %zu returned", k, runs_started, runs_returned);
        CHECK(half == (int)(k & 1), "run(%zu) on half %d", k, half);
        runs_started++;
        if (k >= n) return MIC_ERR_INTERNAL;
        downs[k] = &down;
        CHECK(uploads == std::min(k + 2, n), "run(%zu) after %zu uploads", k, uploads);
        CHECK(ups[k] && ups[k]->pending.load() == 0, "run(%zu): its upload is still in flight", k);
        CHECK(ups[k] && ups[k]->error.load() == 0, "run(%zu): its upload had failed", k);
        if (k >= 2) CHECK(downs[k - 2]->pending.load() == 0, "run(%zu): the download of part %zu is still in flight", k, k - 2);
        if (k >= 2) CHECK(downs[k - 2]->error.load() == 0, "run(%zu): the download of part %zu had failed", k, k - 2);
        CHECK(next_up == (k + 1 < n ? ups[k + 1] : nullptr), "run(%zu): next_up is not the request of upload(%zu)", k, k + 1);
        fake_transfer(down, !(what == "down" && k == fk), 10);   // (slower than two uploads: without the wait for down[k - 2] it is in flight at run(k))
        fake_transfer(down, true, 1);
        runs_returned++;
        if (what == "run" && k == fk) { failed = true; return kRunErr; }
        return MIC_OK;
    });
    // on return nothing is in flight: every request had pending == 0, so every fake transfer has counted itself
    const int completed = g_completed.load();
    CHECK(completed == g_submitted, "%d of %d transfers were complete at the return", completed, g_submitted);
    for (auto &t : g_helpers) t.join();

    // what the protocol makes of the failure
    size_t want_uploads = n, want_runs = n; int want_rc = MIC_OK;
    if (what == "upload") { want_uploads = fk + 1; want_runs = fk ? fk - 1 : 0; want_rc = kUploadErr; }
    else if (what == "run") { want_uploads = std::min(fk + 2, n); want_runs = fk + 1; want_rc = kRunErr; }
    else if (what == "up") { want_uploads = fk + 1; want_runs = fk; want_rc = MIC_ERR_DEVICE; }                              // seen at step 1 of part fk
    else if (what == "down") { want_uploads = std::min(fk + 4, n); want_runs = std::min(fk + 2, n); want_rc = MIC_ERR_DEVICE; }   // seen at step 3 of part fk + 2, or at the end
    else if (what != "none") { fprintf(stderr, "unknown failure %s\n", what.c_str()); return 2; }
    if (what != "none" && fk >= n) { fprintf(stderr, "part %zu of %zu\n", fk, n); return 2; }
    CHECK(uploads == want_uploads, "%zu uploads, expected %zu", uploads, want_uploads);
    CHECK(runs_started == want_runs && runs_returned == want_runs, "%zu runs started, %zu returned, expected %zu", runs_started, runs_returned, want_runs);
    CHECK(rc == want_rc, "returned %d, expected %d", rc, want_rc);
    if (g_bad) return 1;
    printf("ok\n");
    return 0;
}
