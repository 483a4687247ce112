"""CPU model of the split two-state tANS decode (csrc/mic_decode_ls.hip: k_dec_tans_ls_split).

A restatement, in plain Python, of the decode table (tests/table_routes.py: dtable), of the two-state decode loop
(fse2state.go:203-308) and of the split rule: where part 1 starts, the states it starts with, the overlap W, the meeting test and
the count check.  For an oracle-made stream `Stream.split(W)` predicts what the kernel records in MicUnit.split -- outcome, i_sync,
j_sync -- exactly, and `Stream.gate` which units k_dec_classify puts on the split list.

Positions are counts of unread bits: the decoder reads bits [p - n, p) and moves to p - n; bits below 0 read as zeros."""
import numpy as np

import table_routes as R

NOT_TRIED, DONE, NOT_MET, BAD_COUNT, NO_ROOM = range(5)
MIN_TOKENS, OVERLAP, MIN_BITS16 = 131072, 32768, 144          # MicSplitCfg's defaults (csrc/mic_dev.h)
CHUNK = 64
_PAD = 16                                                       # zero bytes in front of the stream: reads below bit 0


class Stream:
    """a two-state FSE stream of `tok` as the oracle writes it, and the decoder's view of it"""

    def __init__(self, mico, tok, req_tl=0):
        tok = np.ascontiguousarray(tok, np.uint16)
        self.tok, self.count = tok, int(tok.size)
        rc, self.blob = mico.fse_compress_tl(tok, 2, req_tl)
        frc, f = mico.fse_stream_facts(tok, 2, req_tl, want_norm=True)
        assert rc == 0 and frc == 0, (rc, frc)
        self.table_log, self.zero_bits, self.hdr_len = f["table_log"], f["zero_bits"], f["hdr_len"]
        tab_sym, dt = R.dtable(f["norm"][:f["symbol_len"]], self.table_log)
        self.tab_sym = tab_sym
        self.new_state = [int(v) & 0xFFFF for v in dt]
        self.nb = [int(v) >> 16 for v in dt]
        bs = self.blob[self.hdr_len:]
        assert bs and bs[-1] != 0
        self.nbytes = len(bs)
        self.bits = 8 * (len(bs) - 1) + bs[-1].bit_length() - 1         # below the end marker
        self._b = bytes(_PAD) + bs + bytes(8)

    # ---- the bit reader and one symbol ----
    def read(self, p, n):
        """bits [p - n, p) as a number, n <= 24"""
        lo = p - n + 8 * _PAD
        if lo < 0:
            return 0
        return (int.from_bytes(self._b[lo >> 3:(lo >> 3) + 4], "little") >> (lo & 7)) & ((1 << n) - 1)

    def start(self, p):
        """the two states read at position p as initial states are (fse2state.go:210-212) -> (p', s0, s1)"""
        tl = self.table_log
        return p - 2 * tl, self.read(p, tl), self.read(p - tl, tl)

    def run(self, p, s, i, n, out=None):
        """n symbols from symbol index i on (state i & 1 reads first); s = [s0, s1] is updated in place -> p"""
        nb, ns, read = self.nb, self.new_state, self.read
        for k in range(i, i + n):
            c = s[k & 1]
            if out is not None:
                out.append(c)
            b = nb[c]
            s[k & 1] = ns[c] + read(p, b)
            p -= b
        return p

    def decode(self):
        """the plain decode -> (symbols, unread bits at the end)"""
        p, s0, s1 = self.start(self.bits)
        st = []
        p = self.run(p, [s0, s1], 0, self.count, st)
        return self.tab_sym[np.asarray(st, np.int64)], p

    # ---- the split rule ----
    def gate(self, min_tokens=MIN_TOKENS, min_bits16=MIN_BITS16):
        return (self.table_log == 13 and not self.zero_bits and self.count >= max(min_tokens, 128)
                and 128 * self.nbytes >= min_bits16 * self.count)

    def split_start(self, W):
        wb = min(W * self.bits // self.count, self.bits)
        return (self.bits + wb) // 2

    def split(self, W=OVERLAP, cap=None):
        """(outcome, i_sync, j_sync) of the kernel for overlap W; cap: tokens of the scratch slab (default: enough)"""
        T = self.count
        W &= ~63
        wc, j_sync = W // CHUNK, W
        if wc >= T // CHUNK + 2:
            return NOT_MET, 0, j_sync
        pm = self.split_start(W)
        p1, a, b = self.start(pm)
        s1 = [a, b]
        p1 = self.run(p1, s1, 0, j_sync)                                 # part 1 after Wc chunks: the meeting point
        # part 0: its last chunk start above p1 (every chunk start before part 1 has got there)
        p, a0, b0 = self.start(self.bits)
        s = [a0, b0]
        snap = (0, p, list(s))
        for c in range(T // CHUNK + 2):
            if c >= wc and p <= p1:
                break
            snap = (c, p, list(s))
            p = self.run(p, s, c * CHUNK, CHUNK)
        c, p, s = snap
        i, met = c * CHUNK, False
        for _ in range(CHUNK + 1):
            if p < p1:
                break
            if p == p1:
                met = s[i & 1] == s1[0] and s[(i + 1) & 1] == s1[1]
                break
            p = self.run(p, s, i, 1)
            i += 1
        if not met:
            return NOT_MET, 0, j_sync
        j_end = T - i + j_sync
        room = (min(cap, T) if cap is not None else T) & ~63
        if i > (T // CHUNK) * CHUNK or j_end > room:
            return NO_ROOM, i, j_sync
        # the over-read rule at the stream's last symbol (bitreader.go:113-120), on part 1's own count
        if self.run(p1, list(s1), j_sync, j_end - j_sync) < 0:
            return BAD_COUNT, i, j_sync
        return DONE, i, j_sync

    def meeting_distance(self, start_bit, s0, s1, limit):
        """symbols a decoder started at `start_bit` with states (s0, s1) runs before it has fallen in with the true decode (same
        position, same states, role by role), or None within `limit`: the measurement behind W and G"""
        true = getattr(self, "_true", None)
        if true is None:                                                 # the true decode: position -> (states at it, reader first)
            true = self._true = {}
            p, a, b = self.start(self.bits)
            s = [a, b]
            for i in range(self.count):
                true[p] = (s[i & 1], s[(i + 1) & 1])
                p = self.run(p, s, i, 1)
        p, s = start_bit, [s0, s1]
        for j in range(limit):
            t = true.get(p)
            if t is not None and t == (s[j & 1], s[(j + 1) & 1]):
                return j
            p = self.run(p, s, j, 1)
            if p < 0:
                break
        return None
