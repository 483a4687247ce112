"""Two-state frame streams for the round of k_dec_tans_ls<2, ZB, TL> (csrc/mic_decode_ls.hip, LS_CHUNK2), made on the CPU
(tests/test_gpu_tans2_round.py).

The round takes its 32-bit window from three ring dwords read a round EARLIER, at the position of that time, and the second state's
offset from the first state's table entry.  What can go wrong is therefore a matter of how far the position moves from one round to
the next and where it stands against the dword grid -- so the streams here put the extremes next to each other:
  * rare_frame: three adjacent tokens whose symbols the stream holds once: tableLog bits each (build_ctable's rule, restated in
    decode_class_streams.worst_chunk_dwords), so one round takes 2 * tableLog bits and the pair beside it straddles two rounds;
  * still_frame: a stream with 0-bit table entries whose dominant token comes sixteen times in a row (rounds that do not move the
    position at all), each such stretch directly followed by a pair of rare tokens (the largest step);
  * decode_class_streams.deep_image at tableLog 15 / 16: chunks that take (nearly) the whole per-chunk budget off the ring;
  * uneven_batch: a wave whose streams differ by whole chunks beside a wave of one stream and its clones.

An image is made from its RESIDUALS: the frame codec predicts a pixel as avg(left, top) (left on row 0, top in column 0, 0 at the
corner: predict_px, oracle/mic_oracle_core.c) and codes 127 + (pixel - prediction) for eight-bit pixels, so running the predictor
forward over a chosen field of residuals gives the image whose tokens are those residuals -- with the run-length layer on top
(rle_encode there): three equal symbols open a run, a run is written as (count, symbol) and a long one in pieces of 124, a literal
chunk as 127 + n and its n symbols.  A run of 124 m symbols of residual -3 (symbol 124) is therefore m pairs (124, 124): 2 m equal
tokens in a row, which is the only way this token format has of repeating a token more than twice.

Nothing here knows what the library thinks of a stream; every property above is asserted from the oracle's tokens and from
fse_stream_facts(..., want_norm=True)."""
import numpy as np

import decode_class_streams as D

THR = 127                         # eight-bit pixels: symbol = THR + residual, |residual| < THR
DOMINANT = 124                    # the piece length of a long run AND the symbol of residual -3
STILL_PAIRS = 8                   # (124, 124) pairs per stretch: sixteen equal tokens in a row


def _rows_for(table_log, w):
    """rows of a frame of about a token per pixel that holds just over min_tokens(table_log) tokens"""
    return -(-D.min_tokens(table_log) // w) + 1


def _forward(w, h, exact, res, level):
    """the image whose residual at (x, y) is res[y, x] where exact[y, x], and level[y, x] otherwise (a pixel set to a value)"""
    ex, rs, lv = exact.tolist(), res.tolist(), level.tolist()
    img = [[0] * w for _ in range(h)]
    for y in range(h):
        row, top, exr, rsr, lvr = img[y], img[y - 1] if y else None, ex[y], rs[y], lv[y]
        for x in range(w):
            if x and y:
                pred = (row[x - 1] + top[x]) >> 1
            elif x:
                pred = row[x - 1]
            elif y:
                pred = top[0]
            else:
                pred = 0
            v = pred + rsr[x] if exr[x] else lvr[x]
            if not exr[x] and v - pred == -3:                               # (a set pixel never makes the dominant symbol)
                v += 1
            assert 0 <= v <= 255 and abs(v - pred) < THR, (x, y, v, pred)
            row[x] = v
    return np.array(img, np.uint16)


# ---- case 1: rounds of 2 * tableLog bits ----------------------------------------------------------------------------------
RARE_PLACES = 8


def rare_residuals(p):
    """the three residuals of place p: 24 values over the places, all different, none under 62 in size"""
    return (62 + 6 * p, -(64 + 6 * p), 66 + 6 * p)


def rare_frame(table_log, seed):
    """noise of twenty levels around 120, and RARE_PLACES places of three adjacent pixels with the residuals rare_residuals(p)
    (signs turned where the pixel would leave the range) -- rows apart, at columns of both parities"""
    w = 1000 - 7 * (seed % 5)
    h = _rows_for(table_log, w)
    exact = np.zeros((h, w), bool)
    res = np.zeros((h, w), np.int64)
    level = 110 + D._noise(w * h, seed, 21).reshape(h, w)
    for p in range(RARE_PLACES):
        y = 2 + p * (h - 4) // RARE_PLACES
        x = 40 + 113 * p + (p & 1)
        exact[y, x:x + 3] = True
        res[y, x:x + 3] = rare_residuals(p)
    return _forward(w, h, exact, res, level)


def rare_triples(mico, stream, req_tl):
    """token indices i at which tokens i, i + 1, i + 2 each have a normalised count <= 1 (tableLog bits each)"""
    tok = mico.delta_rle_compress(stream.img, stream.maxv)
    rc, f = mico.fse_stream_facts(tok, stream.flavour, req_tl, want_norm=True)
    assert rc == 0 and f["table_log"] == stream.table_log
    rare = f["norm"][tok] <= 1
    return [int(i) for i in np.flatnonzero(rare[:-2] & rare[1:-1] & rare[2:])]


# ---- case 2: rounds of no bits at all, then the largest step ---------------------------------------------------------------
STILL_PLACES = 4


def still_frame(table_log, seed, shift=0):
    """two pixels of three have residual -3 (symbol 124: two tokens of three, so its table has 0-bit entries), the third is set to a
    level of its own and breaks every run; at STILL_PLACES places 124 * STILL_PAIRS pixels in a row have residual -3 -- STILL_PAIRS
    pairs (124, 124) -- and the run behind them has a length and a residual the frame holds nowhere else: a pair of rare tokens.
    `shift`: the second place starts that many groups of three pixels later (three tokens more in front of it)"""
    w = 999
    h = _rows_for(table_log, w) + 2 + -(-STILL_PLACES * DOMINANT * STILL_PAIRS // w)   # (a stretch's pixels make few tokens)
    x = np.arange(w)
    exact = np.broadcast_to(x % 3 != 2, (h, w)).copy()
    res = np.full((h, w), -3, np.int64)
    level = 60 + D._noise(w * h, seed, 41).reshape(h, w)
    exact[:, 0] = False                                                     # (column 0 is predicted from above alone: it would sink for ever)
    ex, rs = exact.reshape(-1), res.reshape(-1)
    for p in range(STILL_PLACES):
        y = 3 + p * (h - 6) // STILL_PLACES
        p0 = y * w + 3 * (20 + 37 * p + (shift if p == 1 else 0))                                      # behind a set pixel: the run of -3 starts here
        n = DOMINANT * STILL_PAIRS
        ex[p0:p0 + n] = True
        length, resid = 41 + 5 * p + (p >> 1), 50 + 4 * p                   # tokens (length, 127 + resid): residual length - 127 is met nowhere
        ex[p0 + n:p0 + n + length] = True
        rs[p0 + n:p0 + n + length] = resid
        ex[p0 + n + length] = False                                         # (a set pixel ends the rare run)
    return _forward(w, h, exact, res, level)


def still_places(mico, stream, req_tl):
    """token indices i with tokens i - 2 * STILL_PAIRS .. i - 1 all DOMINANT and tokens i, i + 1 of normalised count <= 1"""
    tok = mico.delta_rle_compress(stream.img, stream.maxv)
    rc, f = mico.fse_stream_facts(tok, stream.flavour, req_tl, want_norm=True)
    assert rc == 0 and f["table_log"] == stream.table_log and f["zero_bits"] == 1
    assert 2 * int((tok == DOMINANT).sum()) > tok.size                      # the dominant token: over half of all
    rare = f["norm"][tok] <= 1
    dom = np.concatenate([[0], np.cumsum(tok == DOMINANT)])
    n = 2 * STILL_PAIRS
    return [int(i) for i in range(n, tok.size - 1) if dom[i] - dom[i - n] == n and rare[i] and rare[i + 1]]


# ---- case 4: chunks that take the whole budget off the ring -------------------------------------------------------------------
def deep_frame(table_log, seed):
    """sixteen bits.  tableLog 16: decode_class_streams.deep_image as the class tests use it.  tableLog 15 has half the table cells
    and every symbol needs one, so its bands of wild rows are narrower: 10 rows in the middle and the last 6 -- some 13 000 values
    the frame holds once or twice, fifteen bits each, and a chunk of 128 of them takes 60 dwords"""
    if table_log == 16:
        return D.deep_image(1000, 270, seed)
    w, h = 1000, 135
    y, x = np.mgrid[0:h, 0:w]
    img = 20000 + 8 * x + 16 * y + D._noise(w * h, seed, 64).reshape(h, w)
    wild = 16384 + (D._mix(w * h, seed + 1) >> np.uint64(40)).astype(np.int64).reshape(h, w) % 32768
    band = np.zeros(h, bool)
    band[h // 3: h // 3 + 10] = True
    band[h - 6:] = True
    return np.where(band[:, None], wild, img).astype(np.uint16)


# ---- the streams, built once per process ------------------------------------------------------------------------------------
_cache = {}


def stream(mico, kind, table_log):
    """kind: 'rare' | 'still' | 'deep' (tableLog 15 and 16) | 'noisy'"""
    key = (kind, table_log)
    if key not in _cache:
        if kind == "rare":
            s = D.Stream(mico, rare_frame(table_log, 7 + table_log), 255, 2, table_log)
        elif kind == "still":
            for shift in (0, 1):                                            # until the rare pairs start at tokens of both parities
                s = D.Stream(mico, still_frame(table_log, 11 + table_log, shift), 255, 2, table_log)
                if len({i & 1 for i in still_places(mico, s, table_log)}) == 2:
                    break
        elif kind == "deep":
            s = D.Stream(mico, deep_frame(table_log, 5 + table_log), 65535, 2, table_log)
        else:
            s = D.Stream(mico, D.plain_image(993, _rows_for(table_log, 993), 3 + table_log, 38), 255, 2, table_log)
        assert s.table_log == table_log and s.img.shape[1] <= 1008, (kind, table_log, s.table_log, s.ntok)
        _cache[key] = s
    return _cache[key]


def uneven_batch(mico):
    """tableLog 13 (three streams per wave, three waves per group): a wave whose streams are 0, 2 and 5 whole chunks over the fewest
    tokens that grant tableLog 13, the shortest in the middle slot, and a second wave of one stream beside its clones"""
    if "uneven" not in _cache:
        base = -(-D.min_tokens(13) // D.CHUNK)
        counts = [(base + 2) * D.CHUNK + 5, base * D.CHUNK + 5, (base + 5) * D.CHUNK + 5, (base + 1) * D.CHUNK + 77]
        units = []
        for i, n in enumerate(counts):
            make = lambda w, h, s=900 + i, a=9 + 6 * i: D.plain_image(w, h, s, a)
            units.append(D.Stream(mico, D.frame_with_tokens(mico, n, make, 1000 - 11 * i), 255, 2, 13))
        assert [u.ntok for u in units] == counts and all(u.table_log == 13 for u in units)
        _cache["uneven"] = units
    return _cache["uneven"]
