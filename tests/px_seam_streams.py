"""Hand-written token streams that put an escape pair, a chain of delimiters, a segment or a piece of a row on every seam of the two
tokens-to-pixels kernels (tests/test_px_seams_cpu.py, tests/test_gpu_px_seams.py): k_dec_pixels_wg (csrc/mic_decode_px.hip, phases 1-3)
and k_dec_rows_tok (csrc/mic_decode_fused.hip).

Three parts, none of which knows the kernels' code paths from the inside:
  * a token WRITER: items ('run', n, value) / ('lit', [symbols]) -> tokens.  Token 0 is the RLE maximum (the delimiter of the frame's
    depth), midCount follows from it (header_walk_streams.mid_count), a header h <= midCount is a run (count, value), a larger one a
    literal chunk of h - midCount symbols (rledecompressu16.go:59-85);
  * a plain DECODER written from the reference's line numbers: tokens -> symbols and their segments, symbols -> pixels
    (deltarlecompressu16.go:69-128), which also says of every symbol whether it is a marker, a payload or plain;
  * a MODEL of both kernels' geometry -- tiles, the marker state carried between them, the LDS segment table and its reloads, the
    prefetch; rows, pieces, escapes, slack, the refusals -- that predicts MicUnit.px_paths and which units k_dec_rows_tok takes.
What a stream MEANS is the oracle's business: its status, token count and pixel hash per case are on record in
tests/golden/px_seam_cases.json (make_golden below), and the CPU test holds the plain decoder to the oracle's pixels.

Filler symbols are thr + a zero-sum pattern of small steps behind a first pixel well inside the range, so every stream
entropy-codes and no filler pixel wraps around 16 bits; a raw pixel behind an escape is the same value or the delimiter itself."""
import bisect
import json
import os

import numpy as np

import header_walk_streams as HW

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "px_seam_cases.json")

# ---- the kernels' constants, each with the line it restates ----
PX_T = 8192                       # mic_decode_px.hip: #define PX_T 8192 -- symbols per tile
PX_THREADS = 1024                 # mic_decode_px.hip: #define PX_THREADS 1024 -- entries of the LDS segment table (s_segx / s_segy)
PX_SPT = 8                        # mic_decode_px.hip: #define PX_SPT (PX_T / PX_THREADS) -- symbols per thread; 64 threads: 512 per wave
PX_WAVE = 64 * PX_SPT             # symbols per wave of the marker scan
PX_STEP = PX_THREADS - PX_SPT     # mic_decode_px.hip: r0 += PX_THREADS - PX_SPT -- reload rounds overlap by 8 segments
RF_SLACK = 512                    # mic_decode_fused.hip: #define RF_SLACK 512 -- symbols behind a row's pixels the escape path looks at
ROWS_LO, ROWS_HI = 1008, 2688     # mic_launch.h: MIC_ROWS_LO / MIC_ROWS_HI -- k_dec_rows_tok takes 1009 .. 2688 columns
GATHER_MAX = 8                    # mic_decode_fused.hip, issue(): need_m & 0x100 -- a ninth piece sends the row to the piece-by-piece form
STAGE_PIXELS = 4                  # mic_dev.h: MIC_STAGE_PIXELS
# mic_dev.h: MIC_PXP_*
PLAIN_TILE, SCAN_TILE, SCAN_ENTRY1, TABLE_RELOAD, PREFETCH = 1, 2, 4, 8, 16
ROW_GATHER, ROW_PIECEWISE, ROW_ESCAPE, ROW_REDO = 1 << 8, 1 << 9, 1 << 10, 1 << 11
PX_BITS = (PLAIN_TILE, SCAN_TILE, SCAN_ENTRY1, TABLE_RELOAD, PREFETCH)
ROW_BITS = (ROW_GATHER, ROW_PIECEWISE, ROW_ESCAPE, ROW_REDO)
INF = 0xFFFFFFFF

DOORS = ("one_state", "two_state")  # k_dec_tans_serial and k_dec_pixels_wg's own walk; k_dec_tans_ls and k_dec_translate's (MIC_STAGE_SEGS)
PLAIN, MARKER, PAYLOAD = 0, 1, 2


def rows_k(w):
    """mic_launch.h: mic_rows_k -- pixels per lane and row of the row kernels' class, 0: another kernel's frame"""
    if w <= ROWS_LO or w > ROWS_HI:
        return 0
    return 18 + 4 * ((max((w + 63) >> 6, 18) - 18 + 3) // 4)


def params(maxv):
    """(depth, delim, thr) of a frame's max value (deltarlecompressu16.go:25-27)"""
    depth = int(maxv).bit_length()
    return depth, (1 << depth) - 1, (1 << (depth - 1)) - 1


# ------------------------------------------------------------------------------------------------------------------ the writer
def write_tokens(maxv, items):
    """items: ('run', n, value[, 'ones']) / ('lit', [symbols][, 'ones']) -> uint16 tokens.  Runs are split at midCount, literal chunks
    at 65535 - midCount; 'ones' writes a run as runs of one and a literal as chunks of one symbol.  Neighbouring literals stay apart."""
    delim = params(maxv)[1]
    t = [delim]
    mid = HW.mid_count(t)
    for it in items:
        ones = len(it) > (3 if it[0] == "run" else 2)
        if it[0] == "run":
            n, v = int(it[1]), int(it[2])
            assert n > 0 and 0 <= v <= 65535
            step = 1 if ones else mid
            while n > 0:
                c = min(n, step)
                t += [c, v]
                n -= c
        else:
            syms = [int(s) for s in it[1]]
            assert syms
            step = 1 if ones else 65535 - mid
            for i in range(0, len(syms), step):
                chunk = syms[i:i + step]
                t.append(mid + len(chunk))
                t += chunk
    return np.array(t, np.uint16)


class Builder:
    """a stream, symbol by symbol: symbol 0 is the max value, `at` the index of the next one"""
    PAT = (1, -1, 0, 2, -2, 0, -1, 1)           # the filler's steps: they sum to zero, so row 0 (left neighbour only) stays level

    def __init__(self, w, h, maxv=4095, first=True):
        self.w, self.h, self.maxv = w, h, maxv
        self.depth, self.delim, self.thr = params(maxv)
        self.level = self.thr * 3 // 4          # the first pixel, and every raw pixel that is not the delimiter
        self.items, self.syms = [], []
        self.lit([maxv, self.thr + self.level] if first else [maxv])   # (first: the first pixel, plain)

    @property
    def at(self):
        return len(self.syms)

    def filler(self, i):
        return self.thr + self.PAT[i % 8]

    def lit(self, syms, ones=False, cut=False):
        syms = [int(s) for s in syms]
        if not syms:
            return self
        last = self.items[-1] if self.items else None
        if last is not None and last[0] == "lit" and (len(last) == 3) == ones and not cut:
            last[1].extend(syms)
        else:
            self.items.append(["lit", list(syms)] + (["ones"] if ones else []))
        self.syms += syms
        return self

    def run(self, n, v, ones=False):
        if n > 0:
            self.items.append(["run", n, int(v)] + (["ones"] if ones else []))
            self.syms += [int(v)] * n
        return self

    def fill(self, n, ones=False, cut=False):
        return self.lit([self.filler(self.at + k) for k in range(n)], ones, cut)

    def fill_to(self, s, **kw):
        assert s >= self.at, (s, self.at)
        return self.fill(s - self.at, **kw)

    def esc(self, raw=None, **kw):
        return self.lit([self.delim, self.level if raw is None else raw], **kw)

    def pixels(self):
        """whole pixels the symbols so far make (a marker at the end still waits for its payload: the next symbol completes its pixel)"""
        n, i, s = 0, 1, self.syms
        while i < len(s):
            i += 2 if s[i] == self.delim else 1
            n += 1
        return n - (1 if i > len(s) else 0)

    def row_start(self, y):
        """fills up to the first symbol of row y"""
        need = y * self.w - self.pixels()
        assert need >= 0
        return self.fill(need)

    def close(self, extra=0, **kw):
        need = self.w * self.h - self.pixels() + extra
        assert need >= 0, need
        return self.fill(need, **kw)


# ------------------------------------------------------------------------------------------------------------------ the plain decoder
def decode_tokens(t, symcap):
    """rledecompressu16.go:59-85, header by header: (symbols, segx, segrun, segy) -- payload token, run flag and first symbol of every
    segment.  The walk stops at the stream's end, or once it holds `symcap` symbols (a frame of N pixels uses 2 N + 1 at most)."""
    t = np.asarray(t, np.uint16)
    mid, pos, out = HW.mid_count(t), 1, 0
    parts, segx, segrun, segy = [], [], [], []
    while pos < t.size and out < symcap:
        h = int(t[pos])
        assert h != 0, "a zero header is the header-walk suite's"
        if h <= mid:
            assert pos + 1 < t.size, "a run without its value is the header-walk suite's"
            parts.append(np.full(h, t[pos + 1], np.uint16))
            n, adv, run = h, 2, True
        else:
            n, adv, run = h - mid, 1 + h - mid, False
            assert pos + adv <= t.size, "a stream that ends inside a literal chunk is the header-walk suite's"
            parts.append(t[pos + 1:pos + adv])
        segx.append(pos + 1); segrun.append(run); segy.append(out)
        out += n
        pos += adv
    syms = np.concatenate(parts) if parts else np.zeros(0, np.uint16)
    return syms, np.array(segx, np.int64), np.array(segrun, bool), np.array(segy, np.int64)


def decode_pixels(syms, w, h):
    """deltarlecompressu16.go:69-128: (pixels or None when the symbols run out, symbols consumed, kind of every symbol, rows in which
    a predicted pixel left 0 .. 65535 before the 16-bit wrap).  Symbol 0 is the max value; a symbol equal to the delimiter takes the
    next one raw, any other is pred + s - thr in uint16 arithmetic, pred = avg / left / top / 0."""
    s = [int(v) for v in syms]
    n = len(s)
    _, delim, thr = params(s[0])
    out = [0] * (w * h)
    kind = np.zeros(n, np.uint8)
    wrapped = set()
    i = 1
    for p in range(w * h):
        if i >= n:
            return None, i, kind, wrapped
        v = s[i]
        if v == delim:
            kind[i] = MARKER
            i += 1
            if i >= n:
                return None, i, kind, wrapped
            kind[i] = PAYLOAD
            val = s[i]
        else:
            y, x = divmod(p, w)
            if x and y:
                pred = (out[p - 1] + out[p - w]) >> 1
            elif x:
                pred = out[p - 1]
            elif y:
                pred = out[p - w]
            else:
                pred = 0
            d = (v - thr) & 0xFFFF
            full = pred + (d - 65536 if d >= 32768 else d)
            if not 0 <= full <= 65535:
                wrapped.add(y)
            val = (pred + v - thr) & 0xFFFF
        out[p] = val
        i += 1
    return np.array(out, np.uint16).reshape(h, w), i, kind, wrapped


def markers(syms, delim):
    """marker[i] = isDelim[i] & !marker[i-1] over ALL symbols (the kernels' recurrence; symbol 0 is no pixel and no delimiter)"""
    d = np.asarray(syms) == delim
    m = np.zeros(len(d), bool)
    prev = False
    for i in range(1, len(d)):
        prev = bool(d[i]) and not prev
        m[i] = prev
    return m


# ------------------------------------------------------------------------------------------------------------------ the model
class Facts:
    """what both kernels see of a case: symbols, segments, counts as the header walks leave them"""

    def __init__(self, tokens, w, h):
        self.w, self.h, self.npx, self.ntok = w, h, w * h, int(len(tokens))
        symcap = 2 * w * h + 2                     # mic_rlewalk.h: symcap = min(u.sym_cap, 2 w h + 2); sym_cap is 4 w h + 80 on decode
        self.syms, self.segx, self.segrun, self.segy = decode_tokens(tokens, symcap)
        self.nseg = len(self.segy)
        self.nsym = min(len(self.syms), symcap)    # MicRleWalk::finish / k_dec_pixels_wg phase 1: nsym = min(out, symcap)
        self.maxv = int(self.syms[0])
        self.depth, self.delim, self.thr = params(self.maxv)
        self.marker = markers(self.syms[:self.nsym], self.delim)
        self.pixels, self.used, self.kind, self.wrapped = decode_pixels(self.syms, w, h)

    def seg_of(self, s):
        return bisect.bisect_right(self.segy, s) - 1


def model_px(f):
    """k_dec_pixels_wg's tile loop: per tile (kind 'plain' / 'scan', entry state, segments that reach into it, table reloaded inside
    it, symbols taken from the prefetch), and the MIC_PXP_* bits"""
    segy = [int(v) for v in f.segy]

    def cover_end(r0):                              # s_segy[PX_THREADS]: first symbol the table's segments do not cover
        return segy[r0 + PX_THREADS] if r0 + PX_THREADS < f.nseg else INF
    notpx = f.marker.copy()
    notpx[0] = True
    isd = np.asarray(f.syms[:f.nsym]) == f.delim
    isd[0] = False
    tiles, bits = [], 0
    carry_px, tab_ok, tab_r0, s_lo, pre_cov = 0, False, 0, 0, False
    base = 0
    while base < f.nsym and carry_px < f.npx:
        end = min(base + PX_T, f.nsym)
        entry = int(f.marker[base - 1]) if base else 0
        reload_, pre = False, pre_cov
        if pre_cov:
            bits |= PREFETCH
        else:
            r0 = tab_r0 if tab_ok else s_lo
            while True:
                if not (tab_ok and r0 == tab_r0):
                    tab_r0, tab_ok = r0, True
                if not cover_end(r0) < end:
                    break
                reload_ = True
                r0 += PX_STEP
        s_lo = f.seg_of(end - 1)
        base2 = base + PX_T
        pre_cov = base2 < f.nsym and cover_end(tab_r0) >= min(base2 + PX_T, f.nsym)
        plain = not isd[base:end].any() and entry == 0
        bits |= PLAIN_TILE if plain else SCAN_TILE | (SCAN_ENTRY1 if entry else 0)
        bits |= TABLE_RELOAD if reload_ else 0
        tiles.append(dict(kind="plain" if plain else "scan", entry=entry, reload=reload_, prefetch=pre,
                          segments=f.seg_of(end - 1) - f.seg_of(base) + 1))
        carry_px += int((~notpx[base:end]).sum())
        base += PX_T
    return dict(tiles=tiles, bits=bits, status=0 if carry_px >= f.npx else -6)


def fetch_form(f, i0):
    """fetch8 of the thread whose symbols begin at i0: ('run' | 'vector' | 'elements', segments its 8 symbols lie in)"""
    tile_end = min((i0 // PX_T + 1) * PX_T, f.nsym)
    wend = min(i0 + PX_SPT, tile_end)
    j = f.seg_of(i0)
    endj = min(int(f.segy[j + 1]) if j + 1 < f.nseg else f.nsym, f.nsym)
    nsegs = f.seg_of(wend - 1) - j + 1
    one = wend - i0 == PX_SPT and i0 + PX_SPT <= endj
    if one and f.segrun[j]:
        return "run", nsegs
    if one and int(f.segx[j]) + (i0 - int(f.segy[j])) + PX_SPT <= f.ntok:
        return "vector", nsegs
    return "elements", nsegs


def model_rows(f):
    """k_dec_rows_tok on a two-state unit: dict(seen, taken, why, rows=[pieces, escapes, used, path, redo], bits)"""
    k = rows_k(f.w)
    if not k:
        return dict(seen=False, taken=False, why="width", rows=[], bits=0)
    ch = k + 8                                      # mic_decode_fused.hip: constexpr int CH = K + 8 -- symbols per lane of the marker scan
    assert 64 * ch == 64 * k + RF_SLACK
    out = dict(seen=True, taken=False, why="", rows=[], bits=0, k=k, ch=ch)
    # mic_decode_fused.hip: if (ntok < 8 || nseg < 1 || nsym < 1 || nseg > 16u * (uint32_t)H + 64u) return;
    if f.ntok < 8 or f.nseg < 1 or f.nsym < 1 or f.nseg > 16 * f.h + 64:
        out["why"] = "unit"
        return out
    spos, bits = 1, 0
    for y in range(f.h):
        if spos + f.w > f.nsym:                     # tokens ran out: the other path's error
            out["why"] = "symbols"
            return out
        pieces = f.seg_of(spos + f.w - 1) - f.seg_of(spos) + 1
        path = "gather" if pieces <= GATHER_MAX else "piecewise"
        row = np.asarray(f.syms[spos:spos + f.w])
        esc, used, nesc, slack_pieces = bool((row >= f.delim).any()), f.w, 0, 0
        if esc:
            have = min(f.w + RF_SLACK, f.nsym - spos)
            st, pl, last = False, 0, None
            for i in range(have):                   # entry state 0: a row starts behind a pixel
                st = int(f.syms[spos + i]) == f.delim and not st
                if st:
                    nesc += 1
                else:
                    pl += 1
                    if pl == f.w:
                        last = i
                        break
            if last is None:                        # total < W: more escapes than the slack holds
                out["why"] = "escapes"
                out["rows"].append(dict(pieces=pieces, escapes=None, used=None, path=path, redo=False, esc=True))
                return out
            used = last + 1
            slack_pieces = f.seg_of(spos + have - 1) - f.seg_of(spos + f.w - 1) + 1 if have > f.w else 0
        redo = y > 0 and y in f.wrapped
        bits |= (ROW_GATHER if path == "gather" else ROW_PIECEWISE) | (ROW_ESCAPE if esc else 0) | (ROW_REDO if redo else 0)
        out["rows"].append(dict(pieces=pieces, escapes=nesc, used=used, path=path, redo=redo, esc=esc, spos=spos, first_seg=f.seg_of(spos),
                                slack_pieces=slack_pieces))
        spos += used
    out["taken"], out["bits"] = True, bits
    return out


def expected_paths(f, door):
    """MicUnit.px_paths and whether MicUnit.dec_stage reads MIC_STAGE_PIXELS"""
    r = model_rows(f) if door == "two_state" else dict(taken=False)
    if r["taken"]:
        return r["bits"], True
    return model_px(f)["bits"], False


# ------------------------------------------------------------------------------------------------------------------ the cases
class Case:
    def __init__(self, name, b, doors=DOORS, **claims):
        self.name, self.w, self.h, self.maxv, self.items, self.doors, self.claims = name, b.w, b.h, b.maxv, b.items, tuple(doors), claims
        self._tokens = self._facts = None

    @property
    def tokens(self):
        if self._tokens is None:
            self._tokens = write_tokens(self.maxv, self.items)
        return self._tokens

    @property
    def facts(self):
        if self._facts is None:
            self._facts = Facts(self.tokens, self.w, self.h)
        return self._facts


PXW, PXH = 300, 84                                  # three tiles and a part


def _px_cases():
    out = []

    def add(name, b, **claims):
        out.append(Case("px/" + name, b, **claims))

    def frame(maxv=4095, w=PXW, h=PXH):
        return Builder(w, h, maxv)
    # ---- an escape pair across a tile, wave or thread edge ----
    for s, tiles in ((8191, {0: "scan0", 1: "scan1"}), (8190, {0: "scan0", 1: "plain"}), (8192, {0: "plain", 1: "scan0"}),
                     (511, {0: "scan0"}), (8192 + 511, {1: "scan0"}), (4103, {0: "scan0"}), (4104, {0: "scan0"})):
        b = frame()
        b.fill_to(s).esc().close()
        add(f"pair_at_{s}", b, markers=[s], payloads=[s + 1], tiles=tiles)
    # ---- chains of delimiters: one RLE run of D, whose parity says which of them are markers ----
    for start in (8185, 8190, 8191, 8192):
        for n in (1, 2, 3, 4, 15, 16):
            b = frame()
            b.fill_to(start).run(n, b.delim).close()
            mk = list(range(start, start + n, 2))
            add(f"chain_{n}_at_{start}", b, markers=mk, payloads=[m + 1 for m in mk], run_at=start)
        b = frame()
        b.fill_to(start).lit([b.delim] * 15).close()
        mk = list(range(start, start + 15, 2))
        add(f"chain_15_literal_at_{start}", b, markers=mk, payloads=[m + 1 for m in mk])
    for start in (5, 6):                            # whole tiles of delimiters, both parities at the tile edges
        b = frame()
        b.fill_to(start).run(2 * PX_T + 1, b.delim).close()
        mk = list(range(start, start + 2 * PX_T + 1, 2))
        add(f"long_chain_at_{start}", b, markers=[mk[0], mk[len(mk) // 2], mk[-1]], payloads=[mk[-1] + 1],
            tiles={0: "scan0", 1: "scan%d" % ((PX_T - 1 - start) % 2 == 0), 2: "scan%d" % ((2 * PX_T - 1 - start) % 2 == 0)})
    # ---- depths ----
    for maxv in (255, 3000, 2047, 2048, 65535):
        b = frame(maxv)
        b.fill_to(8191).esc().close()
        add(f"depth_{maxv}_pair_at_8191", b, markers=[8191], payloads=[8192], tiles={0: "scan0", 1: "scan1"}, delim=params(maxv)[1])
    # ---- ends ----
    b = frame()
    b.fill(PXW * PXH - 2).esc()
    add("last_pixel_escape", b, status=0, markers=[PXW * PXH], last_token_is_payload=True)
    b = frame()
    b.fill(PXW * PXH - 2).lit([b.delim])
    add("last_pixel_escape_without_payload", b, status=-6)
    for e in (0, 1, 2):
        b = frame(w=273, h=30)
        for k in range(e):
            b.fill_to(100 * (k + 1)).esc()
        b.close()
        add(f"npx_8190_escapes_{e}", b, last_symbol=8190 + e, ntiles=1 if e < 2 else 2)
    # ---- surplus: the stream goes on for more than a tile behind the last pixel ----
    b = frame()
    b.close().fill(3000).run(40, b.delim).fill(6000).run(7, b.delim).fill(500)
    add("surplus", b, surplus=PX_T + 1, ntiles=4, tiles={3: "scan0"})
    # ---- dense segments ----
    for with_esc in (False, True):
        b = frame()
        for g in range((PXW * PXH - 9) // 3):       # (three pixels a group)
            b.run(2, b.thr)
            if with_esc and g % 97 == 96:
                b.lit([b.delim], cut=True).lit([b.level], cut=True)
            else:
                b.lit([b.filler(b.at)], cut=True)
        b.close(cut=True)
        add("dense_run2_lit1" + ("_escapes" if with_esc else ""), b, reload=True, min_segments_per_tile=5400)
        b = frame()
        for g in range(PXW * PXH - 9):
            if with_esc and g % 97 == 50:
                b.lit([b.delim, b.level], ones=True)
            else:
                b.fill(1, ones=True)
        b.close(ones=True)
        add("dense_ones" + ("_escapes" if with_esc else ""), b, reload=True, min_segments_per_tile=PX_T)
    # ---- the three fetch forms of a thread's 8 symbols (the thread at symbol 4096) ----
    b = frame()
    b.fill_to(4090).run(64, b.thr).close()
    add("fetch_inside_run", b, fetch=(4096, "run", 1))
    b = frame()
    for k in range(7):                              # 25200 pixels + symbol 0 + 7 markers: the last thread's 8 symbols end the stream
        b.fill_to(100 * (k + 1)).esc()
    b.close()
    add("fetch_vector_ends_at_last_token", b, fetch=(PXW * PXH, "vector", 1), vector_ends_stream=True)
    b = frame()
    b.fill_to(4100).run(40, b.thr).close()
    add("fetch_over_2_segments", b, fetch=(4096, "elements", 2))
    b = frame()
    b.fill_to(4098).run(3, b.thr).close()
    add("fetch_over_3_segments", b, fetch=(4096, "elements", 3))
    b = frame()
    b.fill_to(4096, cut=True)
    for k in range(4):
        b.run(1, b.thr).fill(1, cut=True)
    b.close(cut=True)
    add("fetch_over_8_segments", b, fetch=(4096, "elements", 8))
    # ---- the other predictors behind the raw bits: k_dec_predict_rows (one state only: two states go to k_dec_rows_tok), k_dec_predict2 ----
    for w, h, doors in ((1100, 23, ("one_state",)), (2700, 10, DOORS)):
        b = frame(w=w, h=h)
        b.fill_to(8191).esc().close()
        out.append(Case(f"px/pair_at_8191_{w}x{h}", b, doors, markers=[8191], payloads=[8192], tiles={0: "scan0", 1: "scan1"}))
        b = frame(w=w, h=h)
        b.fill_to(8185).run(15, b.delim).close()
        mk = list(range(8185, 8200, 2))
        out.append(Case(f"px/chain_15_at_8185_{w}x{h}", b, doors, markers=mk, payloads=[m + 1 for m in mk]))
    return out


def _rows_cases():
    out = []
    TWO = ("two_state",)

    def add(name, b, **claims):
        out.append(Case(f"rows/{name}_{b.w}", b, TWO, **claims))
    for w, h in ((1100, 8), (2688, 8)):
        k = rows_k(w)
        ch = k + 8
        wide = w == 2688

        def frame(hh=h, maxv=4095, first=True):
            return Builder(w, hh, maxv, first)
        # ---- escapes in one row ----
        for e in (1, 511, 512, 513, w):
            for y in (0, h // 2, h - 1):
                b = frame(first=y > 0)
                b.row_start(y)
                for _ in range(e):
                    b.esc()
                b.close()
                add(f"escapes_{e}_row_{y}", b, taken=e <= RF_SLACK, row={y: dict(escapes=e if e <= RF_SLACK else None)},
                    **({"have": w + RF_SLACK} if (e, y) == (512, h - 1) else {}))
        # ---- a pair and a chain across a lane chunk of the scan (the row has an escape in front, so it takes the scan) ----
        for l in ((1, 32, 63) if wide else (1, 32, 62, 63)):   # (at 1100 columns lane 61 holds the last symbols of the slack: 62 CH = W + 512)
            y = h // 2
            b = frame()
            b.row_start(y)
            s0 = b.at
            b.esc().fill_to(s0 + ch * l - 1).esc().close()
            add(f"pair_at_lane_{l}", b, taken=True, markers=[s0, s0 + ch * l - 1], row={y: dict(esc=True)})
            b = frame()
            b.row_start(y)
            s0 = b.at
            b.esc().fill_to(s0 + ch * l - 4).run(5, b.delim).close()
            mk = [s0 + ch * l - 4, s0 + ch * l - 2, s0 + ch * l]
            add(f"chain_5_to_lane_{l}", b, taken=True, markers=mk, payloads=[s0 + ch * l + 1], row={y: dict(esc=True)})
        # ---- pieces per row ----
        b = frame(maxv=65535)                       # (midCount 32767: a run may be longer than two rows)
        b.fill(w // 2).run(3 * w, b.thr).close()
        add("one_piece_inside_a_run", b, taken=True, row={2: dict(pieces=1, path="gather")}, row_is_run=2)
        b = frame()
        b.close()
        add("one_literal", b, taken=True, row={y: dict(pieces=1, path="gather", esc=False) for y in range(h)}, nseg=1)
        for p in (2, 8, 9, 12):
            y = 3
            b = frame()
            b.row_start(y)
            size = w // p
            for q in range(p):
                n = size if q < p - 1 else w - size * (p - 1)
                if q % 2 == 0:
                    b.run(n, b.thr)
                else:
                    b.fill(n, cut=True)
            if p % 2 == 0:
                b.close()
            else:
                b.close(cut=True)
            add(f"pieces_{p}", b, taken=True, row={y: dict(pieces=p, path="gather" if p <= 8 else "piecewise")})
        y = 3
        b = frame()
        b.row_start(y)
        s0 = b.at
        b.run(200, b.thr).fill_to(s0 + 401, cut=True).run(206, b.thr).close(cut=True)
        add("piece_ends_mod_8", b, taken=True, row={y: dict(pieces=4, path="gather")}, piece_ends=(y, [200, 401, 607]))
        for n in (1, 3, 7):
            b = frame()
            b.row_start(y)
            s0 = b.at
            b.fill_to(s0 + 801).run(n, b.thr).close(cut=True)
            add(f"piece_of_{n}_inside_a_vector", b, taken=True, row={y: dict(pieces=3, path="gather")}, piece_ends=(y, [801, 801 + n]))
    # ---- at 1100 columns only ----
    w = 1100
    # have cut short by the stream's end
    b = Builder(w, 8)
    b.row_start(7)
    for _ in range(300):
        b.esc()
    b.close()
    add("escapes_300_last_row_nothing_behind", b, taken=True, row={7: dict(escapes=300)}, have=w + 300)
    # row ends
    b = Builder(w, 8)
    b.row_start(3).fill(w - 1).esc().close()
    add("row_ends_in_escape", b, taken=True, row={3: dict(escapes=1, used=w + 1), 4: dict(esc=False)})
    b = Builder(w, 8)
    b.row_start(3).fill(w - 1).esc().esc().close()
    add("row_ends_and_next_begins_in_escape", b, taken=True, row={3: dict(escapes=1, used=w + 1), 4: dict(escapes=1, used=w + 1)})
    b = Builder(w, 8)
    b.row_start(3).fill(w - 1).esc(raw=b.delim).esc().close()           # ... D D | D x ...
    add("row_ends_in_raw_delimiter", b, taken=True, row={3: dict(escapes=1, used=w + 1), 4: dict(escapes=1, used=w + 1)})
    # the refusal by segment count: nseg = 16 H + 64 is taken, one more is not
    for extra in (0, 1):
        h = 8
        want = 16 * h + 64 + extra
        b = Builder(w, h)
        b.fill(9)
        while len(b.items) < want - 1:
            if b.items[-1][0] == "lit":
                b.run(3, b.thr)
            else:
                b.fill(3, cut=True)
        b.close(cut=True)                           # (the last segment)
        add(f"segments_16h_plus_{64 + extra}", b, taken=extra == 0, nseg_delta=extra)
    # the segment window: 24 rows of 7 pieces, a row's first segment 0, 7 .. 161
    h = 24
    b = Builder(w, h)
    for y in range(h):
        end = 1 + (y + 1) * w
        for q in range(7):
            stop = end if q == 6 else b.at + 150 + q
            if q % 2 == 0:
                b.fill_to(stop, cut=y > 0 or q > 0)
            else:
                b.run(stop - b.at, b.thr)
    add("window_24_rows_of_7", b, taken=True, row={y: dict(pieces=7, first_seg=7 * y) for y in range(h)}, nseg=7 * h)
    # a run's value among the first and among the last eight tokens
    b = Builder(w, 8)
    b.items, b.syms = [["lit", [b.maxv]]], [b.maxv]
    b.run(500, b.thr + 1).close(cut=True)
    add("first_row_starts_in_a_run", b, taken=True, run_value_token=("first", 4))
    b = Builder(w, 8)
    b.fill(w * 8 - 300 - 1).run(300, b.thr)
    add("stream_ends_in_a_run", b, taken=True, run_value_token=("last", 1))
    # both special forms at once
    y = 3
    b = Builder(w, 8)
    b.row_start(y)
    b.esc(cut=True)
    size = w // 9
    for q in range(7):
        if q % 2 == 0:
            b.run(size, b.thr)
        else:
            b.fill(size, cut=True)
    b.close(cut=True)
    add("escape_row_of_9_pieces", b, taken=True, row={y: dict(pieces=9, path="piecewise", esc=True)})
    b = Builder(w, 8)
    b.row_start(y).esc().row_start(y + 1)
    for q in range(12):
        if q % 2 == 0:
            b.run(30, b.thr)
        else:
            b.fill(30, cut=True)
    b.close(cut=True)
    add("escape_row_slack_of_many_pieces", b, taken=True, row={y: dict(esc=True, path="gather")}, slack_pieces=(y, 9))
    # no row of eight pieces or fewer: the gather is never taken
    b = Builder(w, 8)
    while b.at + 200 < w * 8:
        b.run(100, b.thr).fill(100, cut=True)
    b.close(cut=True)
    add("every_row_piece_by_piece", b, taken=True, row={y: dict(path="piecewise") for y in range(8)})
    # a pixel that wraps around 16 bits: the row is done again lane by lane
    b = Builder(w, 8)
    b.row_start(y).fill(500).lit([b.thr - 1800]).close()
    add("wrap_around_in_a_row", b, taken=True, row={y: dict(redo=True), y - 1: dict(redo=False)})
    return out


_cases = None


def cases():
    global _cases
    if _cases is None:
        _cases = _px_cases() + _rows_cases()
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)


def ids():
    """(case name, door) of every run"""
    return [(c.name, d) for c in cases() for d in c.doors]


# ------------------------------------------------------------------------------------------------------------------ coding
_coded = {}


def coded(mico, name, door):
    """(w, h, blob, expected dec_kernel, oracle status, oracle pixels or None) of a case through a door; rc 0 of fse_compress and
    the door's kernel are asserted: no case may drop out"""
    key = (name, door)
    if key not in _coded:
        c = case(name)
        rc, blob, facts = HW.code(mico, c.tokens, door)
        assert rc == 0, (name, door, rc)
        rc_o, want = mico.decompress_single_frame(blob, c.w, c.h)
        _coded[key] = (c.w, c.h, blob, HW.expected_kernel(door, facts), rc_o, want)
    return _coded[key]


def golden():
    return json.load(open(GOLDEN))


def escape_heavy(mico, door):
    """(image, blob, expected dec_kernel, tokens) of a frame an encoder writes with two tokens a pixel: a checkerboard of 0 and the
    maximum, every pixel but the first an escape.  Its tokens do not fit the small (tier 1) token slab of a session,
    pixels + pixels / 8 + 4096 (csrc/mic_session.h: tok_cap_tier), and its alphabet is a handful of symbols: only the token count
    can send the batch to the large slabs -- which a one-state stream does not carry in front."""
    y, x = np.mgrid[0:PXH, 0:PXW]
    img = (((x + y) & 1) * 4095).astype(np.uint16)
    tok = mico.delta_rle_compress(img, 4095)
    rc, blob, facts = HW.code(mico, tok, door)
    assert rc == 0, (door, rc)
    return img, blob, HW.expected_kernel(door, facts), tok


def make_golden(mico):
    """tests/golden/px_seam_cases.json from this project's oracle: status, token count and FNV-1a of the pixels, per case and door"""
    rec = {}
    for name, door in ids():
        w, h, blob, _, rc, px = coded(mico, name, door)
        rec[f"{name}/{door}"] = dict(status=int(rc), tokens=int(case(name).tokens.size),
                                     pixels_fnv1a64=f"{mico.fnv1a64(px.tobytes()):016x}" if rc == 0 else None)
    with open(GOLDEN, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
        fh.write("\n")
    return rec


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import mico as _mico
    _mico.lib()
    print(len(make_golden(_mico)), "records written to", GOLDEN)
