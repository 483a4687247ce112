"""A plain-integer restatement of the FSE table stage (csrc/mic_tables.hip, csrc/mic_tables_par.h, mic_read_ncount in
csrc/mic_fse_tables.h), written from the reference lines the kernels cite, and of the forks the device takes through it.

    gate / optimal_table_log     fse2state.go:23-42, fsecompressu16.go:465-518
    normalize_primary            fsecompressu16.go:524-571
    normalize_count2             fsecompressu16.go:573-651, with the name of the route it takes
    Fields / header_bytes        fsecompressu16.go:191-289 as a list of bit fields; write_count_serial is the loop as it stands,
                                 32-bit accumulator and all, and says whether a field met `pending + length > 32`
    ctable / dtable (+ rANS)     fsecompressu16.go:329-431, fsedecompressu16.go:198-263, ransu16.go:77-180
    enc_route / dec_route        MicUnit.tb_route as the kernels must leave it (MIC_TBR_*, csrc/mic_dev.h)

Nothing here imports the package under test; tests/test_table_routes_cpu.py holds it against the oracle, case by case."""
import numpy as np

MIN_TL, MAX_TL, DEF_TL = 5, 16, 11
RTB = (0, 473195, 504333, 520860, 550000, 700000, 750000, 830000)
SMALL_SYMS, SMALL_TL = 8192, 13            # the LDS scratch class
SMALLV = 16                                # slots a symbol may have and still be ranked in registers
STAGE_SMALL, STAGE_BIG = 8 * 1024, 40 * 1024
ERR_USE_RLE, ERR_INTERNAL, ERR_INCOMPRESSIBLE = -3, -8, -10

BITS = ("SMALL", "HBM", "RANS", "PRIMARY", "N2_PAR", "N2_UNIFORM", "N2_SERIAL", "W_PAR", "W_SERIAL",
        "P_SMALL", "P_DEFER_TL", "P_DEFER_LEN", "P_DEFER_SYMS", "P_BIG_STAGE", "P_BIG_HBM", "P_WINDOW")
BIT = {name: 1 << i for i, name in enumerate(BITS)}


def names(route):
    return {n for n in BITS if route & BIT[n]}


def high_bits(v):
    return int(v).bit_length() - 1


def high_bits_of(a):
    """high_bits of every entry of an array of integers in [1, 2^53)"""
    return (np.frexp(np.asarray(a, np.float64))[1] - 1).astype(np.int64)


def lanes(flavour):
    return 8 if flavour == 108 else flavour


def gate(n, max_count, flavour):
    """the gates in front of the table stage, in the order of a bare FSECompressU16* call"""
    if n <= 1 or n <= lanes(flavour) - 1:
        return ERR_INCOMPRESSIBLE
    if max_count == n:
        return ERR_USE_RLE
    if max_count == 1 or max_count < (n >> 15):
        return ERR_INCOMPRESSIBLE
    return 0


def optimal_table_log(n, symbol_len, req=0):
    tl = req if req else DEF_TL
    min_bits = min(high_bits(n - 1) + 1, high_bits(symbol_len - 1) + 2) & 0xFF
    max_bits_src = (high_bits(n - 1) - 2) & 0xFF                           # (uint8 arithmetic: wraps for n <= 4)
    if max_bits_src < tl:
        tl = max_bits_src
    if min_bits > tl:
        tl = min_bits
    density = n // symbol_len
    if symbol_len > 512 and density > 16 and tl < 13:
        tl = 13
    elif density > 64 and symbol_len > 256 and tl < 12:
        tl = 12
    elif density > 32 and symbol_len > 128 and tl < 12:
        tl = 12
    if max_bits_src < tl:
        tl = max_bits_src
    return min(max(tl, MIN_TL), MAX_TL)


def normalize_primary(hist, n, tl):
    """-> (norm, second): second = the corner case that hands the unit to normalizeCount2 (norm is then void)"""
    hist = np.asarray(hist, np.uint64)
    scale = 62 - tl
    step = np.uint64((1 << 62) // n)
    low = hist <= np.uint64(n >> tl)
    prod = hist * step
    proba = (prod >> np.uint64(scale)).astype(np.int64)
    rest = np.uint64(1 << (scale - 20)) * np.asarray(RTB + (0,), np.uint64)[np.minimum(proba, 8)]
    bump = (proba < 8) & ((prod - (proba.astype(np.uint64) << np.uint64(scale))) > rest)
    proba = proba + bump
    norm = np.where(hist == 0, 0, np.where(low, -1, proba)).astype(np.int64)
    pos = np.where(norm > 0, norm, 0)
    largest = int(np.argmax(pos)) if pos.max() > 0 else 0                  # the first symbol with the largest proba
    still = (1 << tl) - int(pos.sum()) - int((norm == -1).sum())
    if -still >= (int(norm[largest]) >> 1):
        return norm, True
    norm[largest] += still
    return norm, False


def normalize_count2(hist, n, tl):
    """-> (rc, norm, route names): N2_PAR or N2_SERIAL, with N2_UNIFORM when the second classification pass is taken"""
    size, sl = 1 << tl, len(hist)
    NOT_YET = -2
    total, distributed = n, 0
    low_threshold = total >> tl
    low_one = ((total * 3) & 0xFFFFFFFF) >> (tl + 1)
    norm = [0] * sl
    for i, c in enumerate(hist):
        c = int(c)
        if c == 0:
            continue
        if c <= low_threshold:
            norm[i] = -1; distributed += 1; total -= c
        elif c <= low_one:
            norm[i] = 1; distributed += 1; total -= c
        else:
            norm[i] = NOT_YET
    route = set()
    if distributed >= size:                                                # the reference divides by zero or spins: no behaviour to match
        return ERR_INTERNAL, None, route
    to_distribute = size - distributed
    if total // to_distribute > low_one:
        route.add("N2_UNIFORM")
        low_one = (total * 3) // (to_distribute * 2)
        for i, c in enumerate(hist):
            if norm[i] == NOT_YET and int(c) <= low_one:
                norm[i] = 1; distributed += 1; total -= int(c)
        if distributed >= size:
            return ERR_INTERNAL, None, route
        to_distribute = size - distributed
    # at most symbol_len symbols can have been distributed: the reference's `distributed == symbolLen + 1` branch is dead code
    assert distributed <= sl
    if total == 0:
        route.add("N2_SERIAL")
        if not any(v > 0 for v in norm):
            return ERR_INTERNAL, None, route                              # the reference loops for ever
        i = 0
        while to_distribute > 0:
            if norm[i] > 0:
                to_distribute -= 1; norm[i] += 1
            i = (i + 1) % sl
        return 0, np.asarray(norm, np.int64), route
    route.add("N2_PAR")
    v_step_log = 62 - tl
    mid = (1 << (v_step_log - 1)) - 1
    r_step = (((1 << v_step_log) * to_distribute) + mid) // total
    tmp = mid
    for i, c in enumerate(hist):
        if norm[i] == NOT_YET:
            end = (tmp + int(c) * r_step) & 0xFFFFFFFFFFFFFFFF
            weight = ((end >> v_step_log) & 0xFFFFFFFF) - ((tmp >> v_step_log) & 0xFFFFFFFF)
            if weight < 1:
                return ERR_INTERNAL, None, route
            norm[i] = weight
            tmp = end
    return 0, np.asarray(norm, np.int64), route


def normalize(hist, n, tl):
    """-> (rc, norm, normaliser route names)"""
    norm, second = normalize_primary(hist, n, tl)
    if not second:
        return 0, norm, {"PRIMARY"}
    return normalize_count2(hist, n, tl)


class Fields:
    """writeCount as bit fields.  Per WRITTEN symbol (every non-zero count and the first zero of a zero run), in symbol order:
    `ones` one-bits of run code (16 per 24 further zeros, 2 per 3), a 2-bit remainder when the symbol closes a run (rem2 >= 0),
    then the count field `value` in `flen` bits.  `start` is the bit position of the symbol's first bit, `cstart` of its count field."""

    def __init__(self, norm, tl):
        v = np.asarray(norm, np.int64)
        sl, size = v.size, 1 << tl
        prev = np.concatenate([[1], v[:-1]])
        written = (v != 0) | (prev != 0)
        closes = (v != 0) & (prev == 0)
        first_zero = (v == 0) & (prev != 0)
        idx = np.arange(sl)
        fz = np.maximum.accumulate(np.where(first_zero, idx, -1))            # the last first-zero at or before s
        R = np.where(closes, idx - fz - 1, 0)                                # zeros of the run beyond its first
        remaining = size + 1 - (np.cumsum(np.abs(v)) - np.abs(v))
        assert int(np.abs(v).sum()) == size and remaining.min() >= 1
        hb = np.minimum(tl, high_bits_of(remaining))
        threshold = 1 << hb
        mx = 2 * threshold - 1 - remaining
        cnt = v + 1
        cnt = np.where(cnt >= threshold, cnt + mx, cnt)
        flen = hb + 1 - (cnt < mx)
        w = np.flatnonzero(written)
        self.tl, self.symbol_len = tl, sl
        self.sym = w
        self.R = R[w]
        self.closes = closes[w]
        self.ones = np.where(self.closes, 16 * (self.R // 24) + 2 * ((self.R % 24) // 3), 0)
        self.rem2 = np.where(self.closes, (self.R % 24) % 3, -1)
        self.value, self.flen = cnt[w], flen[w]
        self.remaining = remaining[w]
        length = self.ones + 2 * self.closes + self.flen
        self.start = 4 + np.cumsum(length) - length
        self.cstart = self.start + self.ones + 2 * self.closes
        self.bits = int(4 + length.sum())
        self.nbytes = (self.bits + 7) >> 3

    def header_bytes(self):
        """the fields laid end to end, LSB first: the header, wherever the reference's 32-bit accumulator drops nothing"""
        k = self.sym.size
        seg_len = np.stack([self.ones, 2 * self.closes, self.flen], 1).ravel()
        seg_val = np.stack([np.zeros(k, np.int64), np.maximum(self.rem2, 0), self.value], 1).ravel()
        seg_one = np.stack([np.ones(k, bool), np.zeros(k, bool), np.zeros(k, bool)], 1).ravel()
        seg_len = np.concatenate([[4], seg_len]); seg_val = np.concatenate([[self.tl - MIN_TL], seg_val]); seg_one = np.concatenate([[False], seg_one])
        first = np.cumsum(seg_len) - seg_len
        j = np.arange(int(seg_len.sum())) - np.repeat(first, seg_len)       # bit number inside its segment
        bit = np.where(np.repeat(seg_one, seg_len), 1, (np.repeat(seg_val, seg_len) >> np.minimum(j, 62)) & 1).astype(np.uint8)
        return np.packbits(bit, bitorder="little").tobytes()


def write_count_serial(norm, tl):
    """the reference's loop as it stands -> (header bytes, wraps): wraps = a count field arrived with `pending + length > 32`,
    where the 32-bit accumulator may drop its top bits (fsecompressu16.go:260-262)"""
    M32 = 0xFFFFFFFF
    norm = [int(x) for x in norm]
    out = bytearray()
    size = 1 << tl
    bit_stream, bit_count = tl - MIN_TL, 4
    remaining, threshold, nb_bits = size + 1, size, tl + 1
    charnum, previous0, wraps = 0, False, False

    def flush():
        nonlocal bit_stream, bit_count
        out.append(bit_stream & 0xFF); out.append((bit_stream >> 8) & 0xFF)
        bit_stream >>= 16; bit_count -= 16

    while remaining > 1:
        if previous0:
            start = charnum
            while norm[charnum] == 0:
                charnum += 1
            while charnum >= start + 24:
                start += 24
                bit_stream = (bit_stream + (0xFFFF << bit_count)) & M32
                out.append(bit_stream & 0xFF); out.append((bit_stream >> 8) & 0xFF)
                bit_stream >>= 16
            while charnum >= start + 3:
                start += 3
                bit_stream = (bit_stream + (3 << bit_count)) & M32
                bit_count += 2
            bit_stream = (bit_stream + ((charnum - start) << bit_count)) & M32
            bit_count += 2
            if bit_count > 16:
                flush()
        count = norm[charnum]
        charnum += 1
        mx = (2 * threshold - 1) - remaining
        remaining -= abs(count)
        count += 1
        if count >= threshold:
            count += mx
        used = nb_bits - (1 if count < mx else 0)
        if bit_count + used > 32:
            wraps = True
        bit_stream = (bit_stream + (count << bit_count)) & M32
        bit_count += used
        previous0 = count == 1
        assert remaining >= 1
        while remaining < threshold:
            nb_bits -= 1; threshold >>= 1
        if bit_count > 16:
            flush()
    out.append(bit_stream & 0xFF); out.append((bit_stream >> 8) & 0xFF)
    n = len(out) - 2 + (bit_count + 7) // 8
    assert charnum <= len(norm)
    return bytes(out[:n]), wraps


def spread(norm, tl):
    """tableSymbol by the reference's serial walk (fsecompressu16.go:341-362)"""
    size = 1 << tl
    step, mask = (size >> 1) + (size >> 3) + 3, size - 1
    table = np.zeros(size, np.int64)
    high = size - 1
    for s in np.flatnonzero(np.asarray(norm) == -1):
        table[high] = s; high -= 1
    pos = 0
    for s in np.flatnonzero(np.asarray(norm) > 0):
        for _ in range(int(norm[s])):
            table[pos] = s
            pos = (pos + step) & mask
            while pos > high:
                pos = (pos + step) & mask
    assert pos == 0
    return table


def _slots(norm):
    return np.where(np.asarray(norm) == -1, 1, np.maximum(norm, 0)).astype(np.int64)


def ctable(norm, tl):
    """buildCTable -> (state_tab[size], tt_nb[symbol_len] as u32, tt_find[symbol_len], the encoder's zero_bits); entries of
    symbols that do not occur are void"""
    norm = np.asarray(norm, np.int64)
    size = 1 << tl
    table = spread(norm, tl)
    state_tab = (size + np.argsort(table, kind="stable")).astype(np.uint32)  # stateTable[cumul[sym]++] = size + position, positions ascending
    slots = _slots(norm)
    total = np.cumsum(slots) - slots
    one = slots == 1
    v1 = np.maximum(slots - 1, 1)
    mbo = tl - high_bits_of(v1)
    tt_nb = np.where(one, (tl << 16) - size, (mbo << 16) - (slots << mbo)) & 0xFFFFFFFF
    tt_find = np.where(one, total - 1, total - slots)
    return state_tab, tt_nb.astype(np.uint32), tt_find.astype(np.int32), int((norm > (size >> 1)).any())


def _next_state_entries(nxt, tl):
    nxt = np.asarray(nxt, np.int64)
    nb = tl - high_bits_of(nxt)
    return (((nxt << nb) - (1 << tl)) | (nb << 16)).astype(np.uint32)


def dtable(norm, tl):
    """buildDtable -> (tab_sym[size], dt[size] = newState | nbBits << 16)"""
    norm = np.asarray(norm, np.int64)
    size = 1 << tl
    table = spread(norm, tl)
    slots = _slots(norm)
    order = np.argsort(table, kind="stable")
    rank = np.empty(size, np.int64)
    rank[order] = np.arange(size) - np.repeat(np.cumsum(slots) - slots, slots)
    return table.astype(np.uint16), _next_state_entries(slots[table] + rank, tl)


def rans_ctable(norm, tl):
    """buildRansEncTable -> (tt_nb = freq | k0 << 20, tt_find = bias) per symbol"""
    norm = np.asarray(norm, np.int64)
    pos = np.maximum(norm, 0); low = (norm == -1).astype(np.int64)
    freq = _slots(norm)
    k0 = tl - high_bits_of(np.maximum(freq, 1))
    bias = np.where(norm == -1, pos.sum() + np.cumsum(low) - low, np.cumsum(pos) - pos)
    return (freq | (k0 << 20)).astype(np.uint32), bias.astype(np.int32)


def rans_dtable(norm, tl):
    """buildRansDecTable -> (tab_sym[size], dt[size]): positives in symbol order, then the low-probability symbols"""
    norm = np.asarray(norm, np.int64)
    pos = np.maximum(norm, 0)
    sym_p = np.repeat(np.arange(norm.size), pos)
    j = np.arange(int(pos.sum())) - np.repeat(np.cumsum(pos) - pos, pos)
    dt_p = _next_state_entries(pos[sym_p] + j, tl)
    lows = np.flatnonzero(norm == -1)
    return (np.concatenate([sym_p, lows]).astype(np.uint16),
            np.concatenate([dt_p, np.full(lows.size, tl << 16, np.uint32)]).astype(np.uint32))


def nbig(norm, flavour):
    return 0 if flavour == 108 else int((np.asarray(norm) > SMALLV).sum())


def scratch(symbol_len, tl):
    return "SMALL" if symbol_len <= SMALL_SYMS and tl <= SMALL_TL else "HBM"


class Unit:
    """everything the model says of one bare FSE unit: hist -> gate, tableLog, counts, header, routes"""

    def __init__(self, hist, flavour, req_tl=0):
        hist = np.asarray(hist, np.int64)
        self.flavour, self.req_tl = flavour, req_tl
        self.n = int(hist.sum())
        self.symbol_len = int(np.flatnonzero(hist)[-1]) + 1
        self.hist = hist[:self.symbol_len]
        self.max_count = int(hist.max())
        self.prefix = 0 if flavour == 1 else 6
        self.rc = gate(self.n, self.max_count, flavour)
        self.norm = self.fields = self.header = None
        self.norm_route, self.wraps = set(), False
        if self.rc:
            return
        self.tl = optimal_table_log(self.n, self.symbol_len, req_tl)
        self.rc, self.norm, self.norm_route = normalize(self.hist, self.n, self.tl)
        if self.rc:
            return
        self.fields = Fields(self.norm, self.tl)
        self.header = self.fields.header_bytes()
        if self.tl == 16:                                                  # a 17-bit field can meet 16 pending bits
            serial, self.wraps = write_count_serial(self.norm, self.tl)
            assert self.wraps or serial == self.header
            self.header = serial
        self.hdr_len = len(self.header)
        assert self.hdr_len == self.fields.nbytes
        self.enc_zero_bits = 0 if flavour == 108 else int((self.norm > (1 << self.tl >> 1)).any())
        self.dec_zero_bits = int((self.norm >= (1 << self.tl >> 1)).any())

    def enc_route(self):
        """MicUnit.tb_route after k_enc_tables_wg (0 for a unit that fails in or in front of the table stage)"""
        if self.rc:
            return 0
        r = BIT[scratch(self.symbol_len, self.tl)] | BIT["W_SERIAL" if self.wraps else "W_PAR"]
        for name in self.norm_route:
            r |= BIT[name]
        if self.flavour == 108:
            r |= BIT["RANS"]
        return r | (nbig(self.norm, self.flavour) << 16)

    def dec_route(self, blob_len):
        """MicUnit.tb_route after k_dec_parse<false>, <true> and k_dec_tables_wg of a blob of blob_len bytes"""
        off, used = self.prefix, self.hdr_len
        r = BIT[scratch(self.symbol_len, self.tl)] | (BIT["RANS"] if self.flavour == 108 else 0) | (nbig(self.norm, self.flavour) << 16)
        given = min(blob_len, STAGE_SMALL) - off                           # bytes the reader is handed
        if self.tl > SMALL_TL:
            r |= BIT["P_DEFER_TL"]
        elif blob_len <= STAGE_SMALL:
            if self.symbol_len <= SMALL_SYMS:
                return r | BIT["P_SMALL"] | (BIT["P_WINDOW"] if given >= 24 else 0)
            r |= BIT["P_DEFER_SYMS"]
        else:
            if self.symbol_len <= SMALL_SYMS and used + 8 < STAGE_SMALL - off:
                return r | BIT["P_SMALL"] | BIT["P_WINDOW"]
            r |= BIT["P_DEFER_LEN"]
        if blob_len <= STAGE_BIG or used + 8 < STAGE_BIG - off:
            return r | BIT["P_BIG_STAGE"] | (BIT["P_WINDOW"] if min(blob_len, STAGE_BIG) - off >= 24 else 0)
        return r | BIT["P_BIG_HBM"]
