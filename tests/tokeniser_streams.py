"""Frames aimed at the seams of k_enc_tokens_wg (csrc/mic_encode.hip), made on the CPU: tests/test_gpu_tokeniser_paths.py encodes
them, tests/test_tokeniser_paths_cpu.py shows without a device that every case reaches the seam it is named for.

A frame is built from a chosen SYMBOL sequence by running the predictor forward, pixel = prediction + symbol - thr, in raster
order.  Where a case forces nothing the pixels follow a noise image (a run-free stretch: the fast tile's food), and a symbol that
would make an accidental triple, or lengthen a forced run, is moved by one.  mico.delta_symbols (the oracle's predictor) confirms
every avg-predictor frame in the CPU test; the gradient predictor's symbols are read back out of the oracle's tokens.

Where things sit: without an escape in front of it, pixel g is symbol g + 1 and is tokenised at window position (g + 3) % 4096 of
pass (g + 3) // 4096 -- thread ((g + 3) % 4096) // 8, position (g + 3) % 8."""
import functools
from collections import namedtuple

import numpy as np

import tokeniser_paths as M

TILE = M.TILE
# sym: the intended stream; expect(counters, trace) -> bool: the seam the case is named for, under the model; aim: what else the
# CPU test checks on the stream itself
Case = namedtuple("Case", "name img maxv pred sym expect aim", defaults=(None,))


def thr_of(maxv):
    return (1 << (int(maxv).bit_length() - 1)) - 1


def px_at(tile, thread, q):
    """the pixel tokenised at position q of `thread` in the pass of `tile` (no escape in front of it)"""
    return tile * TILE + thread * 8 + q - 3


def grad_predict(w, n, nw, ne):
    g = abs(w - nw) + abs(n - nw)
    if g == 0:
        return (w + n) >> 1
    return ((w + n) >> 1) + max(-(g >> 1), min(g >> 1, (ne - nw) >> 3))


def build(W, H, maxv, forced, seed, pred=0, base=None, sigma=None):
    """forced: {pixel: ('s', symbol) | ('e', +1 / -1 / 0: an escape exactly thr above / below / either side of the prediction) | ('p', pixel value)}
    -> (image, the symbol stream it must have)"""
    depth = int(maxv).bit_length()
    thr, delim = thr_of(maxv), (1 << depth) - 1
    base = (maxv + 1) // 2 - (48 if depth >= 12 else 0) if base is None else base
    sigma = (40.0 if depth >= 12 else 3.0 if depth >= 6 else 2.0) if sigma is None else sigma
    noise = np.rint(base + np.random.default_rng(seed).normal(0, sigma, W * H)).astype(np.int64).clip(0, 65535).tolist()
    px, sym = [0] * (W * H), [int(maxv)]
    for g in range(W * H):
        y, x = divmod(g, W)
        if y == 0:
            pr = px[g - 1] if x else 0
        elif x == 0:
            pr = px[g - W]
        elif pred == 0:
            pr = (px[g - 1] + px[g - W]) >> 1
        else:
            nw = px[g - W - 1]
            pr = grad_predict(px[g - 1], px[g - W], nw, px[g - W + 1] if x + 1 < W else nw)
        f = forced.get(g)
        if f is None:
            s = thr + max(1 - thr, min(thr - 1, noise[g] - pr))
            nxt = forced.get(g + 1)
            avoid = nxt[1] if nxt is not None and nxt[0] == "s" else -1
            for t in (0, 1, -1, 2, -2, 3, -3):
                cand = s + t
                if 1 <= cand <= 2 * thr - 1 and 0 <= pr + cand - thr <= 65535 and cand != avoid and not (cand == sym[-1] == sym[-2]):
                    break
            else:
                raise AssertionError(("no free symbol", g))
            v = pr + cand - thr
            sym.append(cand)
        elif f[0] == "s":
            v = pr + f[1] - thr
            sym.append(f[1])
        else:
            v = pr + (f[1] or (1 if pr < thr + 100 else -1)) * thr if f[0] == "e" else f[1]
            if abs(v - pr) >= thr:
                sym += [delim, v]
            else:
                sym.append(thr + v - pr)
        assert 0 <= v <= 65535, (g, v)
        px[g] = v
    return np.asarray(px, np.uint16).reshape(H, W), np.asarray(sym, np.int64)


def run(forced, g, length, symbol):
    for k in range(length):
        forced[g + k] = ("s", symbol)
    return forced


def _case(name, W, H, maxv, forced, expect, seed=1, pred=0, aim=None, **kw):
    img, sym = build(W, H, maxv, forced, seed, pred, **kw)
    return Case(name, img, maxv, pred, sym, expect, aim)


def _routes(trace):
    return [r[4] for r in trace]


# ---- 1: chunk boundaries of the fast tile ------------------------------------------------------------------------------------
def chunk_cases():
    out = []
    T = thr_of(4095); c = T - 3
    for tile, th, bq in [(2, 100, b) for b in range(8)] + [(2, 0, 0), (1, 511, 7), (1, 0, 0), (2, 0, 3), (1, 511, 0)]:
        i_open = tile * TILE + th * 8 + bq - 2                              # the symbol at that position: it must open a chunk
        s0 = i_open % c
        s0 += c if s0 < 8 else 0                                            # the stretch starts there, behind a run of five
        out.append(_case(f"chunk12-t{tile}-th{th}-bq{bq}", 512, 26, 4095, run({}, s0 - 6, 5, T), seed=10 + bq + th, aim=("chunk-opens", tile, th, bq),
                         expect=lambda k, tr: k["fast"] == 2 and k["refused"] == 0 and _routes(tr)[1:3] == ["fast", "fast"]))
    out.append(_case("chunk6-c28", 512, 26, 63, run({}, 40, 5, 31), seed=3, expect=lambda k, tr: k["fast"] == 2 and k["refused"] == 0))
    out.append(_case("gate5-c12", 512, 26, 31, run({}, 40, 5, 15), seed=4,
                     expect=lambda k, tr: k["fast"] == k["refused"] == k["perlane"] == k["serial"] == 0 and k["general"] == 5))
    return out


# ---- 2: into and out of a fast tile --------------------------------------------------------------------------------------------
def border_cases(pred=0):
    out = []
    T = thr_of(4095)
    tag = "g" if pred else ""
    for off in range(-3, 4):                                                # a run of five from symbol 8190 + off: position off of tile 2
        want = (lambda k, tr: k["fast"] == 0 and k["refused"] == 1 and _routes(tr)[1:3] == ["refused", "cool"]) if off <= 0 else \
               (lambda k, tr: k["fast"] == 1 and k["refused"] == 1 and _routes(tr)[1:3] == ["fast", "refused"])
        out.append(_case(f"border{tag}{off:+d}", 512, 26, 4095, run({}, 2 * TILE - 3 + off, 5, T), want, seed=20 + off, pred=pred))
    # the mirror: a run that ends on positions 0 .. 2 of tile 1; the fast path begins when the cool-down is over
    out.append(_case(f"mirror{tag}", 512, 128, 4095, run({}, 3000, TILE - 3 + 3 - 3000, T), seed=28, pred=pred,
                     expect=lambda k, tr: _routes(tr)[:16] == ["general", "refused"] + ["cool"] * 12 + ["fast", "fast"]))
    out.append(_case(f"fast-then-flush{tag}", 512, 24, 4095, {}, seed=29, pred=pred,
                     expect=lambda k, tr: _routes(tr) == ["general", "fast", "fast", "general"] and tr[-1][2] == 0))
    for (W, H) in ((2731, 3), (4097, 2), (1639, 5), (2733, 3)):             # a last tile of 1, 2, 3 and 7 pixels behind a fast one
        r = W * H - 2 * TILE
        out.append(_case(f"fast-then-{r}px{tag}", W, H, 4095, {}, seed=30 + r, pred=pred,
                         expect=lambda k, tr, r=r: _routes(tr) == ["general", "fast", "general", "general"] and tr[2][2] == r))
    return out


# ---- 3: refusal and cool-down -----------------------------------------------------------------------------------------------
def cooldown_cases():
    T = thr_of(4095)
    want = ["general", "fast", "refused"] + ["cool"] * 12 + ["fast"] * 3 + ["general"]
    return [_case("cooldown", 512, 144, 4095, run({}, px_at(2, 200, 2), 3, T), seed=40,
                  expect=lambda k, tr: _routes(tr) == want and k["fast"] == 4 and k["refused"] == 1)]


# ---- 4: escape tiles ----------------------------------------------------------------------------------------------------------
def escape_cases(pred=0):
    tag = "g" if pred else ""
    B = dict(base=2400, pred=pred)                                            # (an escape thr below the prediction stays above 0)

    def esc(name, pixels, H=26, want=lambda k, tr: True, seed=50, extra=None, sign=None):
        f = {g: ("e", sign if sign is not None else +1 if n % 2 == 0 else -1) for n, g in enumerate(pixels)}
        f.update(extra or {})
        return _case(name + tag, 512, H, 4095, f, want, seed=seed, **B)

    T = thr_of(4095)
    out = [
        esc("esc-half0", [TILE + 10 * 8 + 1], want=lambda k, tr: k["esc"] == 1 and k["fast"] == 1 and tr[1][2] == 2049 and tr[2][2] == 2048),
        esc("esc-half1", [TILE + 300 * 8 + 5], want=lambda k, tr: k["esc"] == 1 and tr[1][2] == 2048 and tr[2][2] == 2049),
        esc("esc-255-256", [TILE + 255 * 8 + 7, TILE + 256 * 8], want=lambda k, tr: k["esc"] == 1 and tr[1][2] == tr[2][2] == 2049),
        esc("esc-last-pixel", [2 * TILE - 1], want=lambda k, tr: k["esc"] == 1 and tr[2][2] == 2049),
        esc("esc-partial-tile", [3 * TILE + 1000], want=lambda k, tr: k["esc"] == 1 and k["fast"] == 2 and tr[3][0] == tr[4][0] == 3),
        esc("esc-after-fast", [2 * TILE + 77], want=lambda k, tr: _routes(tr)[:4] == ["general", "fast", "general", "general"] and tr[2][3]),
        esc("esc-before-fast", [TILE + 77], want=lambda k, tr: tr[1][3] and tr[2][3] and _routes(tr)[3] == "fast" and k["refused"] == 0),
        esc("esc-every-pixel", range(512 * 12), H=12, sign=0, want=lambda k, tr: k["esc"] == 2 and tr[0][2] == tr[1][2] == TILE and k["packed"] == 0),
        # residuals of exactly thr - 1 (plain) and thr (an escape), both signs: below row 0 (the packed branch and its way out) and in
        # row 0 (per pixel)
        esc("esc-at-thr", [TILE + 40, TILE + 90, 100, 200], seed=51,
            extra={TILE + 140: ("s", 1), TILE + 190: ("s", 2 * T - 1), 300: ("s", 1), 400: ("s", 2 * T - 1)},
            want=lambda k, tr: k["esc"] == 2),
    ]
    return out


# ---- 5: packed against per-pixel residuals ---------------------------------------------------------------------------------
def packed_cases(pred=0):
    tag = "g" if pred else ""
    out = []
    g = 5 * 512 + 8 * 20 + 7                                                # last pixel of a thread in row 5
    elig = (20 * 512 - 512) // 8

    def w16(k, tr):                                                         # the thread itself, the one behind it, the one below
        return k["packed"] == (0 if pred else elig - 3) and k["kind2"] == 0

    out.append(_case(f"bit15{tag}", 512, 20, 65535, {g: ("p", 33000)}, w16, seed=60, pred=pred, base=30000, sigma=40.0))
    for kz in range(8):                                                     # a row starts at every position of a thread
        out.append(_case(f"rowstart{tag}-W{512 + kz}", 512 + kz, 20, 4095, {}, seed=61 + kz, pred=pred,
                         expect=lambda k, tr, kz=kz: k["kind2"] == (1 if kz else 0) + (1 if (kz * 20) % 8 else 0)))
    for W, H in ((1, 5000), (7, 700), (8, 600), (9, 500)):
        out.append(_case(f"narrow{tag}-W{W}", W, H, 255, {}, seed=70 + W, pred=pred, base=100,
                         expect=lambda k, tr, W=W, H=H: k["kind2"] == ((W * H + 7) // 8 if W < 8 else (W == 9) + (W * H % 8 != 0))))
    for W in range(1001, 1008):                                             # unit tails of 5, 2, 7, 4, 1, 6, 3 pixels
        out.append(_case(f"tail{tag}-{(W * 5) % 8}px", W, 5, 4095, {}, seed=80 + W, pred=pred,
                         expect=lambda k, tr: k["kind2"] == 2))             # the straddling thread and the tail
    return out


# ---- 6: the per-lane write and its thresholds -------------------------------------------------------------------------------
def perlane_cases():
    T = thr_of(4095); c = T - 3
    out = []
    for n in (8, 9, 16, 17):                                                # triples in n threads of wave 2 of tile 0, nothing else
        f = {}
        for e in range(n):
            run(f, px_at(0, 128 + 3 * e, 2), 3, T + 5)
        want = {8: (1, 0, 0), 9: (1, 1, 0), 16: (1, 1, 0), 17: (0, 0, 1)}[n]
        out.append(_case(f"perlane-{n}", 512, 10, 4095, f, seed=90 + n,
                         expect=lambda k, tr, n=n, want=want: tr[0][5][2] == n and sum(tr[0][5]) == n and (k["perlane"], k["round2"], k["serial"]) == want))
    # a run end and the next run's start in one thread; a stretch that starts and closes its chunk in one thread
    f = run(run({}, px_at(0, 200, 3) - 5, 5, T + 1), px_at(0, 200, 3), 5, T + 2)
    run(f, px_at(0, 300, 2) - 5, 5, T + 1); run(f, px_at(0, 300, 4), 5, T + 3)
    out.append(_case("perlane-two-runs", 512, 10, 4095, f, seed=95, expect=lambda k, tr: k["perlane"] >= 2 and k["serial"] == 0))
    for depth_max, cc in ((63, 28), (4095, c)):                             # run-count wraps, run of 2 c + 3 + 10
        L = 2 * cc + 13
        v = thr_of(depth_max)
        for where, first_wrap in (("in-thread", px_at(1, 50, 3)), ("thread-border", px_at(1, 50, 7)), ("tile-border", px_at(2, 0, 0))):
            g0 = first_wrap - (cc + 2)                                     # the run's (c + 3)-th symbol sits there
            H = (g0 + L + 600) // 512 + 1
            out.append(_case(f"wrap-c{cc}-{where}", 512, H, depth_max, run({}, g0, L, v), seed=96,
                             expect=lambda k, tr: k["general"] >= 3, aim=("wraps-at", first_wrap + 3, L, cc)))
    out.append(_case("run-fills-a-tile", 512, 26, 4095, run({}, 4000, 8500, T), seed=97,
                     expect=lambda k, tr: sum(tr[2][5]) == 2 and tr[2][4] != "fast" and tr[2][2] == TILE))   # (the two threads where the count wraps)
    out.append(_case("run-to-the-end", 512, 10, 4095, run({}, 5120 - 6, 6, T), seed=98, expect=lambda k, tr: True, aim=("last-run", 6)))
    return out


# ---- 7: end of stream ---------------------------------------------------------------------------------------------------------
def eos_cases():
    out = []
    npx = 640
    for rem in (0, 1, 2):                                                   # the last stretch has 2 c + rem symbols
        start = npx + 1 - (2 * 28 + rem)                                    # symbol index where it starts
        out.append(_case(f"eos-stretch-{rem}", 64, 10, 63, run({}, start - 1 - 5, 5, 31), seed=100 + rem, expect=lambda k, tr: True, aim=("last-stretch", 2 * 28 + rem)))
    out.append(_case("eos-run-of-2", 64, 10, 63, run({}, npx - 2, 2, 29), seed=104, expect=lambda k, tr: True, aim=("last-run", 2)))
    out.append(_case("eos-run-of-3", 64, 10, 63, run({}, npx - 3, 3, 29), seed=105, expect=lambda k, tr: True, aim=("last-run", 3)))
    return out


# ---- 8: tokens outside the histogram's LDS window -------------------------------------------------------------------------------
def hist_cases():
    # 16 bits: the window is [thr - 4096, thr + 4096).  The delimiter and an escaped 65000 lie above it; the pixels behind the
    # escape are predicted far off, their residuals lie below it: one value of eight outside in a thread of plain literals
    f = {g: ("p", 65000) for g in (TILE + 100, TILE + 3000, 2 * TILE + 5)}
    return [_case("hist16-outside", 512, 26, 65535, f, seed=110, base=30000, sigma=40.0,
                  expect=lambda k, tr: k["esc"] == 2)]


GROUPS = {
    "chunks": chunk_cases,
    "borders": border_cases,
    "cooldown": cooldown_cases,
    "escapes": escape_cases,
    "packed": packed_cases,
    "perlane": perlane_cases,
    "eos": eos_cases,
    "hist": hist_cases,
    "grad": lambda: border_cases(1) + escape_cases(1) + packed_cases(1),
}


@functools.lru_cache(maxsize=None)
def group(name):
    """the cases of one session batch, built once"""
    return tuple(GROUPS[name]())


def model(case):
    """the model's counters and trace of a frame case"""
    h, w = case.img.shape
    return M.predict(case.sym, w, w * h, case.maxv, 0, case.pred, case.img)


# ---- 10: a symbol unit (WaveletV2) ------------------------------------------------------------------------------------------------
def wavelet_frame():
    """128 x 128: flat but for a noisy band of rows -- the detail bands hold long zero runs beside run-free stretches"""
    img = np.full((128, 128), 1000, np.int64)
    img[:40] += np.rint(np.random.default_rng(7).normal(0, 60, (40, 128))).astype(np.int64)
    return img.astype(np.uint16)
