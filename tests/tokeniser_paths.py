"""Which routes k_enc_tokens_wg (csrc/mic_encode.hip) takes through a unit, restated in numpy for the tests -- the encoder's
counterpart of decode_class_streams.dec_cls.  Nothing here makes a token: tokens always come from the oracle.

The input is the unit's delta-symbol stream x[0..M) as the ORACLE gives it (frames: x[0] = maxValue, then one symbol per pixel or
`delim, value` for an escaped pixel; symbol units: the symbols), W, the pixel count and maxValue; the pixels themselves only say
where bit 15 is set.  The facts of the format used:

  * a maximal run of L >= 3 equal symbols is a same-run; it owns a (c, v) pair at every c-th symbol from its (c + 3)-th on and a
    (rem, v) pair at its last symbol, c = midCount - 3; every other symbol owns its literal;
  * symbol 0, and the first symbol behind a same-run, open a literal stretch.

and of the kernel's routing ("Encode"):

  * a tile is 4096 pixels, eight per thread; a tile that holds an escape is walked in two passes (threads 0..255, 256..511), every
    other tile in one; one more pass flushes the last three symbols.  A pass takes n new symbols into its window and tokenises the
    symbols g0 - 3 .. g0 - 3 + n (three behind), g0 = symbols taken before it; thread t owns window positions 8 t .. 8 t + 7;
  * a thread is `lit8` when its eight positions are valid, none of them nor the symbol behind them is in a same-run, none opens a
    stretch, and c >= 16;
  * a full tile without an escape, with c >= 16, g0 >= 6 and a stretch under way in front of it, votes unless a cool-down runs: all
    threads lit8 -> the fast tile; else refused, and the next twelve such tiles do not vote;
  * outside a fast tile a thread with eight valid positions that is not lit8 (c >= 16, not the flush) is a boundary thread; those
    that own a token are written one position per lane in rounds of eight when their wave holds 1..16 of them, by the serial walk
    when it holds more;
  * a thread fetches vectors (kind 1) when its eight pixels exist, W >= 8 and they lie all in row 0 or all below it, else pixel by
    pixel (kind 2); kind 1 takes the packed residuals when the avg predictor is in use, the pixels lie below row 0, none of the
    seventeen samples read (eight pixels, eight above, one to the left) has bit 15 set and none of the eight is an escape."""
import numpy as np

TILE, THREADS, PPT, WAVE, COOL = 4096, 512, 8, 64, 12
NAMES = ("fast", "refused", "esc", "general", "perlane", "round2", "serial", "packed", "kind2")


def mid_count(max_value, src):
    """midCount of the unit's RLE stage: of the delimiter for frames, of maxValue for symbol units"""
    depth = int(max_value).bit_length()
    return (1 << (depth - 1)) - 1


def rle_expand(tok, mid):
    """the symbols a token sequence (headers and payloads only, nothing in front) stands for: a header <= midCount is a run of
    that many of the next word, a larger one is that many literals above midCount"""
    out, i, tok = [], 0, np.asarray(tok, np.int64)
    while i < tok.size:
        h = int(tok[i])
        if h <= mid:
            out.append(np.full(h, tok[i + 1], np.int64)); i += 2
        else:
            out.append(tok[i + 1:i + 1 + h - mid]); i += 1 + h - mid
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def pixel_symbol_counts(x, npx, max_value):
    """frames: symbols per pixel (2 = escaped) from the stream's own delimiters"""
    delim = (1 << int(max_value).bit_length()) - 1
    cnt = np.ones(npx, np.int64)
    cand = np.flatnonzero(np.asarray(x[1:]) == delim) + 1
    # walk the delimiters in order: one that is the value behind an earlier delimiter is payload
    esc_at, skip_until = [], -1
    for s in cand.tolist():
        if s <= skip_until:
            continue
        esc_at.append(s); skip_until = s + 1
    esc_at = np.asarray(esc_at, np.int64)
    px = esc_at - 1 - np.arange(esc_at.size)                                 # every earlier escape shifted the stream by one
    cnt[px] = 2
    assert 1 + int(cnt.sum()) == len(x), (cnt.sum(), len(x))
    return cnt


def symbol_facts(x, c):
    """per symbol: in a same-run, opens a stretch, owns a token"""
    x = np.asarray(x, np.int64)
    m = x.size
    first = np.ones(m, bool); first[1:] = x[1:] != x[:-1]
    starts = np.flatnonzero(first)
    length = np.diff(np.append(starts, m))
    rid = np.cumsum(first) - 1
    same = (length >= 3)[rid]
    k = np.arange(m) - starts[rid] + 1                                       # 1-based index inside the maximal run
    last = np.ones(m, bool); last[:-1] = first[1:]
    wraps = same & (k > 3) & ((k - 3) % c == 0)
    before = np.ones(m, bool); before[1:] = same[:-1]
    sts = ~same & before
    owns = ~same | last | wraps
    return same, sts, owns


def passes(cnt, npx, src):
    """(tile, n new symbols, escape tile, flush) of every pass in order"""
    out = []
    ntiles = (npx + TILE - 1) // TILE
    for t in range(ntiles):
        lo, hi = t * TILE, min(npx, (t + 1) * TILE)
        if cnt is not None and (cnt[lo:hi] == 2).any():
            half = min(hi, lo + TILE // 2)
            out.append((t, int(cnt[lo:half].sum()), True, False))
            out.append((t, int(cnt[half:hi].sum()), True, False))
        else:
            out.append((t, hi - lo, False, False))
    out.append((ntiles, 0, False, True))
    return out


def predict(x, W, npx, max_value, src=0, pred=0, pixels=None):
    """the nine counters (NAMES) of a unit, and a trace of its passes: (tile, g0, n, escape tile, route, boundary threads that own a
    token per wave) with route one of 'fast', 'refused', 'cool', 'general'"""
    x = np.asarray(x, np.int64)
    mid = mid_count(max_value, src)
    c = mid - 3
    cnt = None if src else pixel_symbol_counts(x, npx, max_value)
    same, sts, owns = symbol_facts(x, c)
    m = x.size
    k = dict.fromkeys(NAMES, 0)
    trace = []
    g0 = 0 if src else 1
    cool = 0
    sts_idx = np.flatnonzero(sts)
    p = np.arange(TILE)
    for tile, n, esc, flush in passes(cnt, npx, src):
        nwin = 3 if flush else n
        i = g0 - 3 + p
        valid = (p < nwin) & (i >= 0)
        ii = np.clip(i, 0, m - 1)
        full = valid.reshape(THREADS, PPT).all(1)
        sm = (same[ii] & valid).reshape(THREADS, PPT)
        behind = np.clip(i[PPT - 1::PPT] + 1, 0, m - 1)                      # the symbol behind each thread's eight
        lit8 = full & (c >= 16) & (not flush) & ~sm.any(1) & ~same[behind] & ~(sts[ii] & valid).reshape(THREADS, PPT).any(1)
        route = "general"
        done = sts_idx[sts_idx < g0 - 3]                                     # stretch starts tokenised so far
        str1 = int(done[-1]) + 1 if done.size else 0
        if not flush and not esc and n == TILE and c >= 16 and g0 >= 6 and str1 != 0 and g0 >= str1 + 3:
            if cool:
                cool -= 1; route = "cool"
            elif lit8.all():
                route = "fast"
            else:
                route = "refused"; cool = COOL
        per_wave = [0] * (THREADS // WAVE)
        if route == "fast":
            k["fast"] += 1
        else:
            k["general"] += 1
            k["refused"] += route == "refused"
            cf = full & ~lit8 & (c >= 16) & (not flush) & (owns[ii] & valid).reshape(THREADS, PPT).any(1)
            per_wave = cf.reshape(-1, WAVE).sum(1).tolist()
            for q in per_wave:
                k["perlane"] += 1 <= q <= 16
                k["round2"] += 9 <= q <= 16
                k["serial"] += q > 16
        trace.append((tile, g0, n, esc, route, per_wave))
        g0 += n
    assert g0 == m, (g0, m)
    ntiles = (npx + TILE - 1) // TILE
    k["esc"] = sum(1 for t in range(ntiles) if cnt is not None and (cnt[t * TILE:(t + 1) * TILE] == 2).any())
    # fetch kind and the packed branch, per thread and tile
    gb = np.arange(0, ntiles * TILE, PPT)
    gb = gb[gb < npx]
    whole = gb + PPT <= npx
    if src:
        kind1 = whole
        packed = kind1
    else:
        kind1 = whole & (W >= PPT) & ((gb >= W) | (gb + PPT <= W))
        packed = np.zeros(gb.size, bool)
        if pred == 0:
            px = np.asarray(pixels, np.int64).ravel()
            assert px.size == npx
            for j in np.flatnonzero(kind1 & (gb >= W)).tolist():
                g = int(gb[j])
                hi = (px[g:g + PPT] | px[g - W:g - W + PPT]).max() | px[g - 1]
                packed[j] = hi < 0x8000 and (cnt[g:g + PPT] == 1).all()
    k["packed"] = int(packed.sum())
    k["kind2"] = int((~kind1).sum())
    return {n: int(v) for n, v in k.items()}, trace
