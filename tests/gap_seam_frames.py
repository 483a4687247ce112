"""Frames aimed at the seams of the gap-removal kernels (csrc/mic_gap.hip), and a model of k_enc_gap's walk.  Test infrastructure
only; nothing here calls the code under test.

A single row gives nearly exact control of the set of used token values: the predictor of a row's pixel is its left neighbour, so a
difference d codes as the token thr + d, and the pixels are the running sum of the chosen differences.  Beside those the row's
tokens hold the delimiter, max_value, one count token thr + n per literal chunk of n symbols, a count token c per run of c equal
symbols, and -- behind a step of thr and more, an escape -- the raw pixel.  `walk` orders the wanted differences so that the pixels
stay inside [0, max_value] and pads the row with differences it already has, never the same one twice in a row (no run); `row` takes
the differences as written (the dense cases: runs of 3, 4, 5, ... pixels give the count tokens 3, 4, 5, ...).

What a case IS is read from the oracle's tokens of its frame, never from how it was built: `facts` runs the oracle's tokeniser,
`model` restates the walk of k_enc_gap over the used values -- steps of GAP_CHUNK bins, four waves of 64 threads with four bins each,
the escapes of the delta map and where each escape's predecessor lies -- and tests/test_gap_seams_cpu.py holds every case to the
property in its name and the set to SEAMS.  tests/golden/gap_seam_cases.json (make_golden below) records what the restatement in
tests/gap_ref.py gives for every case and nstates."""
import json
import os
from collections import namedtuple

import numpy as np

import gap_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gap_seam_cases.json")

# ---- the kernels' constants, each with the line it restates (mic_gap.hip) ----
GAP_THREADS = 256                 # #define GAP_THREADS 256
GAP_WAVES = GAP_THREADS // 64     # #define GAP_WAVES (GAP_THREADS / 64)
GAP_CHUNK = GAP_THREADS * 4       # #define GAP_CHUNK (GAP_THREADS * 4): bins per step, four per thread
WAVE_BINS = GAP_CHUNK // GAP_WAVES
ESCAPE = 255                      # gap >= 255: 0xFF + u16
TIER1_SYMS = 8192                 # mic_session.h: tab_syms_tier(1); tier 2: 65536
NSTATES = (2, 4, 8)


def depth_of(maxv):
    return int(maxv).bit_length()


def thr_of(maxv):
    return (1 << (depth_of(maxv) - 1)) - 1


def delim_of(maxv):
    return (1 << depth_of(maxv)) - 1


def hist_hi(maxv):
    """the bins k_enc_gap walks (k_enc_tokens_wg's hist_hi): the 8192-bin window up to depth 13, beyond it the largest token -- the
    delimiter, always one -- plus one"""
    return TIER1_SYMS if depth_of(maxv) <= 13 else delim_of(maxv) + 1


def tier_of(maxv):
    """session_encode_enqueue: max_value >= 1 << 13 starts in tier 2"""
    return 2 if maxv >= (1 << 13) else 1


# ---- the builder ----
def row(maxv, diffs):
    px = np.cumsum(np.asarray(diffs, dtype=np.int64))
    assert px.min() >= 0 and px.max() <= maxv, (int(px.min()), int(px.max()))
    return px.astype(np.uint16).reshape(1, -1)


def walk(maxv, targets, pad=0, seed=1):
    """a row whose differences are exactly {t - thr for t in targets}: each once, in an order that keeps the pixels in range, with
    differences already used in between where none of the rest fits, and `pad` more of them at the end -- drawn so that a
    difference's count falls off with its rank by size, which is what lets a row of several hundred distinct tokens entropy-code"""
    thr = thr_of(maxv)
    need = sorted(set(int(t) - thr for t in targets), key=lambda d: (abs(d), d))
    assert need and all(abs(d) < thr for d in need), "a token a difference cannot give"
    rng = np.random.default_rng(seed)
    weight = 1.0 / (1.0 + np.arange(len(need))) ** 1.5
    rem, out, p, mid = list(need), [], 0, maxv // 2
    while rem or pad > 0:
        fits = [d for d in rem if 0 <= p + d <= maxv]
        if fits:
            d = min(fits, key=lambda d: (abs(p + d - mid), d))
            rem.remove(d)
        else:
            ok = np.array([0 <= p + d <= maxv and d != 0 and not (out and out[-1] == d) for d in need])
            assert ok.any(), (p, rem[:4])
            if rem:                                                       # towards where one of the rest fits
                goal = maxv if min(rem, key=abs) < 0 else 0
                d = min((d for d, k in zip(need, ok) if k), key=lambda d: (abs(p + d - goal), d))
            else:
                pad -= 1
                homing = ok & np.array([abs(p + d - mid) < abs(p - mid) for d in need])
                pick = homing if abs(p - mid) > maxv // 4 and homing.any() else ok
                w = weight * pick
                d = need[int(rng.choice(len(need), p=w / w.sum()))]
        out.append(d)
        p += d
        assert len(out) < 400000
    return row(maxv, out)


def around(maxv, k):
    """the tokens of the differences -k .. k"""
    return list(range(thr_of(maxv) - k, thr_of(maxv) + k + 1))


# ---- the model ----
Escape = namedtuple("Escape", "index value pred gap step wave where idle before first_of_step")


def model(e, hi):
    """k_enc_gap's walk over the sorted used values e < hi: the busy steps, per step the used values per wave, the escapes and, of
    each, where its predecessor lies -- 'wave' (another thread of the same wave), 'step' (another wave of the same step), 'prev' (the
    step before) or 'far' (an earlier step, `idle` steps without a used value between) -- how many escapes the scan has counted
    before it (esc0) and whether it is its step's first used value; and where walk 2 puts each entry of the delta map."""
    e = [int(v) for v in e]
    assert e == sorted(set(e)) and (not e or e[-1] < hi) and hi % GAP_CHUNK == 0
    busy = sorted({v // GAP_CHUNK for v in e})
    per_wave = {s: [0] * GAP_WAVES for s in busy}
    for v in e:
        per_wave[v // GAP_CHUNK][v % GAP_CHUNK // WAVE_BINS] += 1
    escapes, at = [], []
    for i, v in enumerate(e):
        if i == 0:
            at.append(3)
            continue
        p = e[i - 1]
        at.append(5 + (i - 1) + 2 * len(escapes))                       # map[at]: the byte the entry starts at, mode byte included
        if v - p - 1 < ESCAPE:
            continue
        sv, sp = v // GAP_CHUNK, p // GAP_CHUNK
        if sv == sp:
            where = "wave" if v % GAP_CHUNK // WAVE_BINS == p % GAP_CHUNK // WAVE_BINS else "step"
        else:
            where = "prev" if sv == sp + 1 else "far"
        escapes.append(Escape(i, v, p, v - p - 1, sv, v % GAP_CHUNK // WAVE_BINS, where, max(0, sv - sp - 1), len(escapes), sv != sp))
    return dict(steps=hi // GAP_CHUNK, busy=busy, per_wave=per_wave, escapes=escapes, at=at)


def model_delta_map(e, hi):
    """mode || delta map written the way walk 2 writes it: every entry at the position the model gives"""
    m = model(e, hi)
    esc = {x.index for x in m["escapes"]}
    size = 5 + (len(e) - 1) + 2 * len(esc) if len(e) else 5
    out = bytearray(size)
    out[0], out[1], out[2] = gap_ref.MODE_DELTA, len(e) & 0xFF, len(e) >> 8
    for i, v in enumerate(e):
        a = m["at"][i]
        if i == 0:
            out[a], out[a + 1] = v & 0xFF, v >> 8
        elif i in esc:
            g = v - e[i - 1] - 1
            out[a], out[a + 1], out[a + 2] = 0xFF, g & 0xFF, g >> 8
        else:
            out[a] = v - e[i - 1] - 1
    return bytes(out)


def model_compaction(hist, hi, lo_shift=0, hi_shift=0):
    """walk 2's in-place move of the histogram, step by step as the kernel does it: within a step every bin is read before any is
    written; a used bin v keeps its place only inside [c_used, c_used + used_all) -- the indices this step writes -- and is zeroed
    otherwise, then the counts land at their compact indices; in the kernel a thread zeroes its bin and writes its count in one go,
    in no order among threads, so a bin that is both zeroed and written may end either way: such a bin is returned as -1.  Returns
    the slab afterwards.  (lo_shift, hi_shift: the zeroing rule's two ends moved, for the test of the cases)"""
    h = np.array(hist[:hi], dtype=np.int64)
    c_used = 0
    for base in range(0, hi, GAP_CHUNK):
        vals = [v for v in range(base, base + GAP_CHUNK) if h[v]]
        counts = [int(h[v]) for v in vals]
        zeroed = [v for v in vals if v < c_used + lo_shift or v >= c_used + len(vals) + hi_shift]
        for v in zeroed:
            h[v] = 0
        for k, c in enumerate(counts):
            h[c_used + k] = -1 if c_used + k in zeroed else c
        c_used += len(vals)
    return h


# ---- the cases ----
class Case:
    def __init__(self, name, maxv, px, claims):
        self.name, self.maxv, self.px, self.claims = name, maxv, px, claims
        self.h, self.w = px.shape
        self._facts = None

    def facts(self, mico):
        """from the oracle's tokens: tokens, the used values e, hi, the model, and the decision's figures"""
        if self._facts is None:
            tok = mico.delta_rle_compress(self.px, self.maxv)
            e = gap_ref.used_values(tok)
            apply, mode, best, _ = gap_ref.choose(tok)
            sym_len = int(e[-1]) + 1
            raw, delta = 3 + 2 * len(e), gap_ref.delta_map_size(e)
            self._facts = dict(tokens=tok, e=[int(v) for v in e], hi=hist_hi(self.maxv), apply=apply, mode=mode if apply else 0, best=best,
                               chosen=mode, raw=raw, delta=delta, bitmap=3 + (int(e[-1]) + 8) // 8, slack=sym_len - len(e) - 8 * best,
                               half=len(e) < sym_len // 2)
            self._facts["model"] = model(self._facts["e"], self._facts["hi"])
        return self._facts


def _dense(maxv, first, last_run, sparse, pad=1500):
    """tokens first .. 2 by differences of nearly -thr (0: the raw pixel behind an escape down to 0), 3 .. last_run as the counts of
    runs of +1 / -1, then the sparse ones"""
    thr = thr_of(maxv)
    d = []
    if first == 0:
        d += [thr - 1, 1, -thr]                      # 2046, 2047, then an escape down to pixel 0: delimiter, raw 0
    if first <= 1:
        d += [thr - 1, -(thr - 1)]                   # token 1
    if first <= 2:
        d += [thr - 2, -(thr - 2)]                   # token 2
    d += [300]
    for n in range(3, last_run + 1):
        d += [1 if n % 2 else -1] * n
    rest = walk(maxv, sparse, pad=pad)[0].astype(np.int64)
    start = int(np.sum(d))
    d += [int(rest[0]) - start] + [int(v) for v in np.diff(rest)]
    return row(maxv, d)


_cases = None


def cases():
    global _cases
    if _cases is not None:
        return _cases
    c = []

    def add(name, maxv, px, **claims):
        c.append(Case(name, maxv, px, claims))

    def band(maxv):                                   # plain entries, so that the delta map beats the raw one: used > 2 * escapes + 1
        return around(maxv, 12)
    # ---- step, wave and thread edges ----
    add("edges/depth12", 4095, walk(4095, band(4095) + [1023, 1024, 1279, 1280, 3071, 3072, 3400], pad=300),
        pairs={"step": [1023, 3071], "wave": [1279], "thread": [2051]}, mode=0x03)
    add("edges/depth16_late_steps", 65535,
        walk(65535, band(65535) + [1023, 1024, 4000, 61439, 61440, 62719, 62720, 63491, 63492], pad=400),
        pairs={"step": [61439], "wave": [62719], "thread": [63491]}, mode=0x03, only_delimiter_in_step=63)
    # ---- escape thresholds: gaps of 253 .. 256, and one whose two bytes differ ----
    add("escape/thresholds", 4095, walk(4095, band(4095) + [100, 354, 609, 865, 1122, 1687, 3500], pad=300),
        gaps={354: 253, 609: 254, 865: 255, 1122: 256, 1687: 0x234}, mode=0x03)
    # the widest gap one wave can hold is 254, bins 0 and 255 of a wave: an escape's predecessor is never in its own wave
    add("escape/widest_gap_inside_a_wave", 4095, walk(4095, band(4095) + [1280, 1535, 1536, 1791, 3300], pad=300),
        gaps={1535: 254, 1791: 254}, same_wave=[1535, 1791], mode=0x03)
    # ---- where the predecessor of an escape lies ----
    add("escape/predecessor_places", 8191, walk(8191, band(8191) + [100, 3200, 3210, 3600, 5000, 7000], pad=300),
        where={3200: ("far", 2), 4083: ("step", 0), 7000: ("far", 1), 8191: ("prev", 0)}, mode=0x03, last_bin_of_tier1=True)
    add("escape/predecessor_far_depth16", 65535, walk(65535, band(65535) + [2000, 2300, 30000, 30400, 31500, 60000], pad=400),
        where={2300: ("prev", 0), 30000: ("far", 26), 32755: ("prev", 0), 60000: ("far", 25), 65535: ("far", 4)}, mode=0x03,
        only_delimiter_in_step=63)
    # ---- several escapes in one step, escapes carried into a later step ----
    add("escape/four_in_one_step", 8191,
        walk(8191, band(8191) + [1500, 2050, 2051, 2052, 2320, 2321, 2600, 2601, 2603, 2900, 2901, 5200, 5201, 5800, 6500], pad=300),
        in_step={2: [2050, 2320, 2600, 2900]}, first_of_step={5200: 6, 6500: 8}, mode=0x03, last_bin_of_tier1=True)
    add("escape/carried_depth14", 10000,
        walk(10000, band(10000) + [300, 700, 1100, 5000, 5001, 5300, 5301, 5700, 12000, 12001, 12300, 15000], pad=300),
        first_of_step={5000: 2, 12000: 8, 15000: 10}, in_step={5: [5300, 5700]}, mode=0x03, max_value_token=10000)
    # ---- a dense prefix: compact index == value, or three behind it, while the histogram moves in place ----
    add("dense/prefix_from_0", 4095, _dense(4095, 0, 120, [1100, 1600, 1601, 2500, 3000, 3001, 3500]), dense=(0, 120, 137), mode=0x03)
    add("dense/prefix_from_3", 4095, _dense(4095, 3, 120, [1100, 1600, 1601, 2500, 3000, 3001, 3500]), dense=(3, 120, 132), mode=0x03)
    # every token in step 0 (depth 10), the bins numUsed - 1 and numUsed themselves used, and numUsed a multiple of four: the two bins
    # at the end of what walk 2 must keep.  Nothing is written behind them, and k_enc_hist_clean clears [0, numUsed) in vectors of
    # four bins, so with numUsed % 4 == 0 a bin left dirty at numUsed stays dirty for the slot's next frame
    add("dense/one_step_depth10", 1023, _dense(1023, 0, 59, [75, 76, 400, 500, 600, 700], pad=1200), dense=(0, 59, 76), mode=0x03,
        used_is_used=76)
    # ---- the decision: behind a delta map at depth 12, symLen - used - 8 * best = 4064 - 9 * used - 16 * escapes.  A band of
    # consecutive tokens around thr, lone tokens below it (an escape each) and the padding (the count tokens thr + n) set the two
    t = thr_of(4095)
    add("decision/tie_is_not_applied", 4095, walk(4095, list(range(t - 222, t + 222)) + [1500], pad=8000),
        decision=(0, 448, 2, 0x03), mode=0x00)
    add("decision/slack_1_is_applied", 4095, walk(4095, around(4095, 215) + [200, 500, 800, 1100, 1400], pad=8309),
        decision=(1, 439, 7, 0x03), mode=0x03)
    add("decision/raw_equals_delta_takes_raw", 4095, walk(4095, [t - 300, t + 300, t + 301], pad=400), raw_minus_delta=0, mode=0x01)
    add("decision/delta_one_under_raw", 4095, walk(4095, [t - 300, t + 300, t + 301, t + 302], pad=400), raw_minus_delta=1, mode=0x03)
    add("decision/bitmap_is_smallest", 4095, walk(4095, around(4095, 300), pad=6000), mode=0x00, chosen=0x02)
    # ---- depths and tiers ----
    add("depth/14_not_a_power_of_two", 9999,
        walk(9999, band(9999) + [1023, 1024, 8000, 8400, 9215, 9216, 14000, 14335, 14336], pad=300),
        mode=0x03, max_value_token=9999, pairs={"step": [1023, 9215, 14335]})
    _cases = c
    assert len({x.name for x in c}) == len(c)
    return c


def case(name):
    return next(c for c in cases() if c.name == name)


def names():
    return [c.name for c in cases()]


# ---- what the set must reach, and what it reaches by the model ----
SEAMS = (
    "step_edge_depth12", "wave_edge_depth12", "thread_edge_depth12", "step_edge_depth16_late", "wave_edge_depth16_late",
    "thread_edge_depth16_late", "gap_253", "gap_254", "gap_255", "gap_256", "escape_bytes_differ", "widest_gap_inside_a_wave",
    "pred_other_wave", "pred_previous_step", "pred_two_idle_steps", "three_escapes_one_step_plain_between",
    "later_step_starts_with_escape_carried", "dense_prefix_index_equals_value", "dense_prefix_index_trails_value",
    "decision_tie_not_applied", "decision_least_slack_applied", "decision_raw_equals_delta", "decision_delta_one_under_raw",
    "decision_bitmap_smallest", "depth_12", "depth_13_delimiter_last_bin_of_tier1", "depth_14_16_steps", "depth_16_64_steps",
    "step_63_only_delimiter", "max_value_not_2k_minus_1", "tier_1", "tier_2", "one_step_bins_used_minus_1_and_used_are_used_and_used_is_4k",
)


def _edge_pairs(e):
    s = set(e)
    return [v for v in e if v + 1 in s]


def seams_of(cs, f):
    """the seams one case reaches, by the model of its oracle tokens alone"""
    e, m, hit = f["e"], f["model"], set()
    depth = depth_of(cs.maxv)
    late = depth == 16
    for v in _edge_pairs(e):
        if depth == 12 or (late and v // GAP_CHUNK >= 48):
            tag = "_depth12" if depth == 12 else "_depth16_late"
            if v % GAP_CHUNK == GAP_CHUNK - 1:
                hit.add("step_edge" + tag)
            elif v % WAVE_BINS == WAVE_BINS - 1:
                hit.add("wave_edge" + tag)
            elif v % 4 == 3:
                hit.add("thread_edge" + tag)
    for a, b in zip(e, e[1:]):
        g = b - a - 1
        if g in (253, 254, 255, 256):
            hit.add("gap_%d" % g)
        if g >= 256 and (g & 0xFF) != (g >> 8) and (g >> 8) and (g & 0xFF):
            hit.add("escape_bytes_differ")
        if g == 254 and a % WAVE_BINS == 0:
            hit.add("widest_gap_inside_a_wave")
    if f["apply"] and f["mode"] == gap_ref.MODE_DELTA:                    # (the escapes are written only into an applied delta map)
        for x in m["escapes"]:
            assert x.where != "wave"
            if x.where == "step":
                hit.add("pred_other_wave")
            if x.where == "prev":
                hit.add("pred_previous_step")
            if x.where == "far" and x.idle >= 2:
                hit.add("pred_two_idle_steps")
            if x.first_of_step and x.before >= 1:
                hit.add("later_step_starts_with_escape_carried")
        for s in m["busy"]:
            xs = [x for x in m["escapes"] if x.step == s]
            plain_between = all(any(a.value < v < b.value for v in e if v - 1 in e) for a, b in zip(xs, xs[1:]))
            if len(xs) >= 3 and len({x.wave for x in xs}) >= 3 and plain_between:
                hit.add("three_escapes_one_step_plain_between")
    if f["apply"]:
        run = 0
        while run + 1 < len(e) and e[run + 1] == e[run] + 1:
            run += 1
        sparse_later = sum(1 for v in e if v // GAP_CHUNK >= 1) >= 4
        if run >= 100 and sparse_later:
            hit.add("dense_prefix_index_equals_value" if e[0] == 0 else "dense_prefix_index_trails_value")
    if depth == 12 and f["chosen"] == gap_ref.MODE_DELTA and f["half"] and len(e) > 1:
        if f["slack"] == 0 and not f["apply"]:
            hit.add("decision_tie_not_applied")
        if f["slack"] == 1 and f["apply"]:
            hit.add("decision_least_slack_applied")
    if f["apply"] and f["raw"] == f["delta"] and f["mode"] == gap_ref.MODE_RAW:
        hit.add("decision_raw_equals_delta")
    if f["apply"] and f["raw"] == f["delta"] + 1 and f["mode"] == gap_ref.MODE_DELTA:
        hit.add("decision_delta_one_under_raw")
    if f["chosen"] == gap_ref.MODE_BITMAP and not f["apply"] and f["half"]:
        hit.add("decision_bitmap_smallest")
    if depth == 12:
        hit.add("depth_12")
    if depth == 13 and cs.maxv == 8191 and e[-1] == TIER1_SYMS - 1 and f["apply"]:
        hit.add("depth_13_delimiter_last_bin_of_tier1")
    if depth == 14 and m["steps"] == 16 and f["apply"]:
        hit.add("depth_14_16_steps")
    if depth == 16 and m["steps"] == 64 and f["apply"]:
        hit.add("depth_16_64_steps")
        if m["per_wave"].get(63) == [0, 0, 0, 1]:
            hit.add("step_63_only_delimiter")
    if f["apply"] and m["busy"] == [0] and len(e) % 4 == 0 and len(e) in e and len(e) - 1 in e and e.index(len(e) - 1) < len(e) - 2:
        hit.add("one_step_bins_used_minus_1_and_used_are_used_and_used_is_4k")
    if cs.maxv & (cs.maxv + 1) and cs.maxv in e:
        hit.add("max_value_not_2k_minus_1")
    hit.add("tier_%d" % tier_of(cs.maxv))
    return hit


# ---- the record ----
def reference(mico, cs, nstates):
    """(rc, blob, info) of the restatement"""
    return gap_ref.compress(mico, cs.px, cs.maxv, nstates)


def golden():
    return json.load(open(GOLDEN))


def record_of(mico, cs, nstates):
    rc, blob, info = reference(mico, cs, nstates)
    return dict(status=rc, mode=info["mode"] if rc == 0 else -1, header_len=info["header_len"] if rc == 0 else 0, blob_len=len(blob),
                blob_fnv1a64=f"{mico.fnv1a64(blob):016x}")


def make_golden(mico):
    """tests/golden/gap_seam_cases.json from this project's oracle and tests/gap_ref.py: status, mode byte, header length, blob length
    and FNV-1a of the blob, per case and nstates"""
    rec = {f"{cs.name}/{ns}": record_of(mico, cs, ns) for cs in cases() for ns in NSTATES}
    with open(GOLDEN, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
        fh.write("\n")
    return rec


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import mico as _mico
    print(len(make_golden(_mico)), "records ->", GOLDEN)


# ---- the decode side: maps no encoder writes, around a small frame's streams ----
def table_log_of(fse):
    off = 6 if fse[0] == 0xFF else 0                                      # N-state streams carry a 6-byte prefix
    return (fse[off] & 0xF) + 5


def small_frames():
    """`shallow`, 40 x 6 pixels of depth 4: every token is below 16, so a bitmap can be two bytes long; `deep`, 200 x 30 of depth 16:
    its plain stream has the delimiter 65535 in it (a smaller frame's plain stream does not entropy-code behind its header)"""
    y, x = np.mgrid[0:6, 0:40]
    shallow = (5 + (x // 9 + y) % 4 + (x % 13 == 5) * 3).astype(np.uint16)
    shallow[3, 20:31] = 6
    y, x = np.mgrid[0:30, 0:200]
    deep = (1000 + (x * 7 + y * 3) % 5).astype(np.uint16)
    deep[4, 30] = 41234
    return (shallow, 15), (deep, 65535)


def _streams(mico, px, maxv):
    """(tokens, used values, the compact tokens' FSE stream, the plain tokens' FSE stream)"""
    tok = mico.delta_rle_compress(px, maxv)
    e = gap_ref.used_values(tok)
    lut = np.zeros(65536, dtype=np.uint16)
    lut[e] = np.arange(len(e), dtype=np.uint16)
    rc, fse = gap_ref.fse_chain(mico, lut[tok])
    rc2, plain = gap_ref.fse_chain(mico, tok)
    assert rc == 0 and rc2 == 0
    return tok, [int(v) for v in e], fse, plain


def delta_map_escaping(e, escaped):
    """gap_ref.delta_map with entry i in the 3-byte form where escaped(i) says so (or the gap needs it)"""
    out = bytearray([len(e) & 0xFF, len(e) >> 8, e[0] & 0xFF, e[0] >> 8])
    for i in range(1, len(e)):
        g = e[i] - e[i - 1] - 1
        out += bytes([0xFF, g & 0xFF, g >> 8]) if g >= 255 or escaped(i) else bytes([g])
    return bytes(out)


_crafted = None


def crafted_maps(mico):
    """-> (pixels of the shallow frame, pixels of the deep one, {name: (stream, frame, the reference's status)})"""
    global _crafted
    if _crafted is not None:
        return _crafted
    (sh, sh_max), (dp, dp_max) = small_frames()
    _, e, fse, plain = _streams(mico, sh, sh_max)
    _, de, dfse, dplain = _streams(mico, dp, dp_max)
    assert e[-1] == 15 and 8 <= len(e) <= 16 and de[-1] == 65535
    m = {}
    # bitmaps of 2 .. 8192 bytes: maxSym declared above the largest used value; the bytes behind the used ones are empty, and so are
    # the lanes of k_dec_gap_map they fall to -- every set bit lies in lane 0's run from 65 bytes on, in lanes 0 and 1 below
    for nbytes in (2, 32, 63, 64, 65, 127, 128, 129, 8192):
        m[f"bitmap/bytes_{nbytes}"] = (b"\x02" + gap_ref.bitmap_map(e, 8 * nbytes - 1), "shallow")
    # maxSym at every residue mod 8, every bit behind it set in the last byte: those are no symbols
    for max_sym in range(16, 24):
        bm = bytearray(gap_ref.bitmap_map(e, max_sym))
        bm[-1] |= (0xFF << (max_sym % 8 + 1)) & 0xFF
        m[f"bitmap/max_sym_{max_sym}"] = (b"\x02" + bytes(bm), "shallow")
    # raw maps with unused entries behind the used ones: one short of tier 1's table, the table, one more, and the format's most
    for n in (8191, 8192, 8193, 65535):
        m[f"raw/entries_{n}"] = (b"\x01" + gap_ref.raw_map(e + [(20000 + 3 * i) & 0xFFFF for i in range(n - len(e))]), "shallow")
        m[f"raw/deep_entries_{n}"] = (b"\x01" + gap_ref.raw_map(de + [(7 * i) & 0xFFFF for i in range(n - len(de))]), "deep")
    # delta maps with none, some and all of the entries escaped; a delta map as long as the format allows
    m["delta/none_escaped"] = (b"\x03" + delta_map_escaping(e, lambda i: False), "shallow")
    m["delta/some_escaped"] = (b"\x03" + delta_map_escaping(e, lambda i: i % 3 == 1), "shallow")
    m["delta/all_escaped"] = (b"\x03" + delta_map_escaping(e, lambda i: True), "shallow")
    m["delta/deep_some_escaped"] = (b"\x03" + delta_map_escaping(de, lambda i: i % 2 == 0), "deep")
    m["delta/long_tail"] = (b"\x03" + delta_map_escaping(e + [16 + 2 * i for i in range(20000)], lambda i: i % 5 == 0), "shallow")
    streams = {k: (v[0] + (fse if v[1] == "shallow" else dfse), v[1]) for k, v in m.items()}
    # the identity maps in front of the PLAIN tokens' stream: the full bitmap, and the delta map of 0 .. 65534 -- one entry short of
    # the deep frame's delimiter, which the payload emits
    full = b"\x02\xff\xff" + b"\xff" * 8192
    ident = b"\x03" + delta_map_escaping(list(range(65535)), lambda i: False)
    streams["bitmap/full"] = (full + plain, "shallow")
    streams["bitmap/deep_full"] = (full + dplain, "deep")
    streams["delta/shallow_0_to_65534"] = (ident + plain, "shallow")
    streams["delta/0_to_65534"] = (ident + dplain, "deep")
    # numSymbols 1: the first entry alone (every other compact symbol is out of range, and emitted)
    streams["delta/num_symbols_1"] = (b"\x03\x01\x00" + bytes([e[0] & 0xFF, e[0] >> 8]) + fse, "shallow")
    streams["delta/deep_num_symbols_1"] = (b"\x03\x01\x00" + bytes([de[0] & 0xFF, de[0] >> 8]) + dfse, "deep")
    out = {}
    for k, (s, which) in streams.items():
        px = sh if which == "shallow" else dp
        out[k] = (s, which, gap_ref.decompress(mico, s, px.shape[1], px.shape[0])[0])
    _crafted = (sh, dp, out)
    return _crafted


def truncations(mico):
    """-> (pixels, {form: (stream, header length)}): one stream of each map form around the shallow frame's compact stream, short
    enough to decode every prefix up to header + 1 in one batch"""
    (sh, sh_max), _ = small_frames()
    _, e, fse, _ = _streams(mico, sh, sh_max)
    maps = {"raw": b"\x01" + gap_ref.raw_map(e), "bitmap": b"\x02" + gap_ref.bitmap_map(e, 15),
            "delta": b"\x03" + gap_ref.delta_map(e), "delta_escaped": b"\x03" + delta_map_escaping(e, lambda i: i % 2 == 1)}
    return sh, {k: (v + fse, len(v)) for k, v in maps.items()}


_wide = None


def wide_alphabet(mico):
    """a row of 153601 pixels at depth 16 with more than 8192 used values, behind its raw map: a COMPACT alphabet only tier 2's
    tables hold.  Differences +-1 .. +-4200, four of each, then a long stretch of +-1.  -> (pixels, stream, used values, tableLog)"""
    global _wide
    if _wide is None:
        d = [30000]
        for k in range(1, 4201):
            d += [k, -k] * 4
        d += [1, -1] * ((153601 - len(d)) // 2)
        px = row(65535, d)
        _, e, fse, _ = _streams(mico, px, 65535)
        _wide = (px, b"\x01" + gap_ref.raw_map(e) + fse, e, table_log_of(fse))
    return _wide
