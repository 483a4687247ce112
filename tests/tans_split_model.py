"""CPU model of the split two-state tANS decode (csrc/mic_decode_ls.hip: k_dec_tans_ls_parts<2> and <4>).

A restatement, in plain Python, of the decode table (tests/table_routes.py: dtable), of the two-state decode loop
(fse2state.go:203-308) and of the split rule for `n` parts (2 or 4; a chunk is 128 / n symbols): where the parts start, the states
they start with, the hand-over after W symbols, the n - 1 joins, the room and count checks, and the routing between the two
instances.  For an oracle-made stream `split_parts` predicts what the kernel records in MicUnit.split -- outcome, I_1 .. I_{n-1} and
the failing boundary -- exactly, `Stream.split` the same as the two-part instance's (outcome, i_sync, j_sync), `joined` the state
sequence k_dec_translate reads out of tok and the scratch regions, and `route` the list k_dec_classify puts a unit on.

Positions are counts of unread bits: the decoder reads bits [p - n, p) and moves to p - n; bits below 0 read as zeros."""
import numpy as np

import table_routes as R

NOT_TRIED, DONE, NOT_MET, BAD_COUNT, NO_ROOM = range(5)
MIN_TOKENS, OVERLAP, MIN_BITS16 = 131072, 32768, 144          # MicSplitCfg's defaults (csrc/mic_dev.h)
MIN_TOKENS4 = 262144                                            # MicSplitCfg::min_tokens4
UNSPLIT, TWO_PARTS, FOUR_PARTS = "class 0", "split", "split4"   # the lists of k_dec_classify a class-0 unit can land on
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
        return starts(self, W, 2)[1]

    def split(self, W=OVERLAP, cap=None):
        """(outcome, i_sync, j_sync) of the two-part instance for overlap W; cap: tokens of the scratch slab (default: enough).
        Its one region is clamped by the stream's own length (LsParts<2>::region)"""
        room = (self.count if cap is None else min(cap, self.count)) & ~63
        outcome, I, _ = split_parts(self, W, R=room, n=2)
        return outcome, I[0], W & ~63

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


def route(s, min_tokens=MIN_TOKENS, min_tokens4=MIN_TOKENS4, min_bits16=MIN_BITS16):
    if not s.gate(min_tokens=min_tokens, min_bits16=min_bits16):
        return UNSPLIT
    return FOUR_PARTS if s.count >= min_tokens4 else TWO_PARTS


def region(px):
    """R, the tokens of a scratch region, of a tier-1 four-part unit of `px` pixels: a third of its token slab, in whole chunks"""
    return ((px + px // 8 + 4096) // 3) & ~31


def starts(s, W, n=4):
    """the bit positions the n parts start at"""
    wb = min(W * s.bits // s.count, s.bits)
    x = (s.bits + (n - 1) * wb) // n
    return [s.bits] + [(n - p) * x - (n - 1 - p) * wb for p in range(1, n)]


class Parts:
    """what the chunk loop of n parts leaves behind: per part the hand-over (position, states) after W steps and the snapshot
    (chunk, position, states) it is joined from; `steps[p]` holds part p's states, step by step, when `keep` is set"""

    def __init__(self, s, W, keep=False, n=4):
        T = s.count
        self.n, self.chunk = n, 128 // n
        self.W = W = W & ~63
        wc, cap = W // self.chunk, T // self.chunk + 2
        self.handed = wc < cap
        self.hand, self.snap, self.steps = [None] * n, [None] * n, [[] for _ in range(n)]
        if not self.handed:
            return
        pos = starts(s, W, n)
        # the hand-overs first: every part's position and states after wc chunks
        for p in range(1, n):
            q, a, b = s.start(pos[p])
            st = [a, b]
            q = s.run(q, st, 0, W)
            self.hand[p] = (q, st[0], st[1])
        for p in range(n):
            q, a, b = s.start(pos[p])
            st = [a, b]
            snap = (0, q, list(st))
            out = self.steps[p] if keep else None
            for c in range(cap):
                if p == n - 1:
                    on = q > 0                                           # bits left
                else:
                    on = c < wc or q > self.hand[p + 1][0]
                if on:
                    snap = (c, q, list(st))
                elif c >= wc:
                    break                                                # (the kernel runs on while a neighbour is on; nothing is read of that)
                q = s.run(q, st, c * self.chunk, self.chunk, out)
            self.snap[p] = snap

    def join(self, s, p):
        """boundary p | p + 1 -> part p's step index where its position and states are part p + 1's hand-over, or None"""
        c, q, st = self.snap[p]
        st = list(st)
        qn, a, b = self.hand[p + 1]
        i = c * self.chunk
        for _ in range(self.chunk + 1):
            if q < qn:
                return None
            if q == qn:
                if i >= (self.W if p else 0) and st[i & 1] == a and st[(i + 1) & 1] == b:
                    return i
                return None
            q = s.run(q, st, i, 1)
            i += 1
        return None


def split_parts(s, W=OVERLAP, R=None, parts=None, n=4):
    """(outcome, (I_1 .. I_{n-1}), failing boundary) of the kernel for overlap W and regions of R tokens (default: enough)"""
    T = s.count
    P = parts or Parts(s, W, n=n)
    W, n, chunk = P.W, P.n, P.chunk
    R = (1 << 30) if R is None else R
    I = [0] * (n - 1)
    if not P.handed:
        return NOT_MET, tuple(I), 1
    at = 0
    for b in range(n - 1):
        e = P.join(s, b)
        if e is None:
            return NOT_MET, tuple(I), b + 1
        at = at + e - W if b else e
        I[b] = at
        if (e > R) if b else (at > (T // chunk) * chunk):
            return NO_ROOM, tuple(I), b + 1
    if I[-1] > T:
        return BAD_COUNT, tuple(I), n
    j_end = T - I[-1] + W
    if j_end > R:
        return NO_ROOM, tuple(I), n
    c, q, st = P.snap[n - 1]
    js = c * chunk
    if j_end > js:
        # the over-read rule at the stream's last symbol (bitreader.go:113-120), on the last part's own count, from its last chunk
        # start with bits left; more than a chunk behind it: the chunk behind the snapshot started without bits
        if j_end - js > chunk or s.run(q, list(st), js, j_end - js) < 0:
            return BAD_COUNT, tuple(I), n
    return DONE, tuple(I), 0


split4 = split_parts                                            # (n = 4 is the default)


def joined(s, W=OVERLAP, n=4):
    """the states k_dec_translate reads of a DONE unit: tok[i] below I_1, then part p's steps W + i - I_p"""
    P = Parts(s, W, keep=True, n=n)
    outcome, I, _ = split_parts(s, W, parts=P)
    assert outcome == DONE, outcome
    bounds = [0, *I, s.count]
    out = list(P.steps[0][:I[0]])
    for p in range(1, n):
        k = bounds[p + 1] - bounds[p]
        seg = P.steps[p][P.W:P.W + k]
        assert len(seg) == k, (p, len(seg), k)
        out += seg
    return out, I
