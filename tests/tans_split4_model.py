"""CPU model of the four-part split of the two-state tANS decode (csrc/mic_decode_ls.hip: k_dec_tans_ls_split4).

On top of tests/tans_split_model.py's stream (decode table, bit reader, one symbol): where the four parts start, the hand-over
after W symbols, the three joins, the room and count checks, and the routing between the two split instances.  For an oracle-made
stream `split4` predicts what the kernel records in MicUnit.split / split4 -- outcome, I_1 .. I_3 and the failing boundary --
exactly, `joined` the state sequence k_dec_translate reads out of tok and the three scratch regions, and `route` the list
k_dec_classify puts a unit on.

Positions are counts of unread bits, as in tans_split_model."""
from tans_split_model import Stream, NOT_TRIED, DONE, NOT_MET, BAD_COUNT, NO_ROOM, MIN_TOKENS, OVERLAP, MIN_BITS16   # noqa: F401

MIN_TOKENS4 = 262144                                            # MicSplitCfg::min_tokens4 (csrc/mic_dev.h)
CHUNK, PARTS = 32, 4
UNSPLIT, TWO_PARTS, FOUR_PARTS = "class 0", "split", "split4"   # the lists of k_dec_classify a class-0 unit can land on


def route(s, min_tokens=MIN_TOKENS, min_tokens4=MIN_TOKENS4, min_bits16=MIN_BITS16):
    if not s.gate(min_tokens=min_tokens, min_bits16=min_bits16):
        return UNSPLIT
    return FOUR_PARTS if s.count >= min_tokens4 else TWO_PARTS


def region(px):
    """R, the tokens of a scratch region, of a tier-1 unit of `px` pixels: a third of its token slab, in whole chunks"""
    return ((px + px // 8 + 4096) // 3) & ~31


def starts(s, W):
    """the bit positions the four parts start at"""
    wb = min(W * s.bits // s.count, s.bits)
    x = (s.bits + 3 * wb) // 4
    return [s.bits] + [(4 - p) * x - (3 - p) * wb for p in (1, 2, 3)]


class Parts:
    """what the chunk loop leaves behind: per part the hand-over (position, states) after W steps and the snapshot
    (chunk, position, states) it is joined from; `steps[p]` holds part p's states, step by step, when `keep` is set"""

    def __init__(self, s, W, keep=False):
        T = s.count
        self.W = W = W & ~63
        wc, cap = W // CHUNK, T // CHUNK + 2
        self.handed = wc < cap
        self.hand, self.snap, self.steps = [None] * PARTS, [None] * PARTS, [[] for _ in range(PARTS)]
        if not self.handed:
            return
        pos = starts(s, W)
        # the hand-overs first: every part's position and states after wc chunks
        for p in range(1, PARTS):
            q, a, b = s.start(pos[p])
            st = [a, b]
            q = s.run(q, st, 0, W)
            self.hand[p] = (q, st[0], st[1])
        for p in range(PARTS):
            q, a, b = s.start(pos[p])
            st = [a, b]
            snap = (0, q, list(st))
            out = self.steps[p] if keep else None
            for c in range(cap):
                if p == PARTS - 1:
                    on = q > 0                                           # bits left
                else:
                    on = c < wc or q > self.hand[p + 1][0]
                if on:
                    snap = (c, q, list(st))
                elif c >= wc:
                    break                                                # (the kernel runs on while a neighbour is on; nothing is read of that)
                q = s.run(q, st, c * CHUNK, CHUNK, out)
            self.snap[p] = snap

    def join(self, s, p):
        """boundary p | p + 1 -> part p's step index where its position and states are part p + 1's hand-over, or None"""
        c, q, st = self.snap[p]
        st = list(st)
        qn, a, b = self.hand[p + 1]
        i = c * CHUNK
        for _ in range(CHUNK + 1):
            if q < qn:
                return None
            if q == qn:
                if i >= (self.W if p else 0) and st[i & 1] == a and st[(i + 1) & 1] == b:
                    return i
                return None
            q = s.run(q, st, i, 1)
            i += 1
        return None


def split4(s, W=OVERLAP, R=None, parts=None):
    """(outcome, (I_1, I_2, I_3), failing boundary) of the kernel for overlap W and regions of R tokens (default: enough)"""
    T = s.count
    P = parts or Parts(s, W)
    W = P.W
    R = (1 << 30) if R is None else R
    I = [0, 0, 0]
    if not P.handed:
        return NOT_MET, tuple(I), 1
    at = 0
    for b in range(3):
        e = P.join(s, b)
        if e is None:
            return NOT_MET, tuple(I), b + 1
        at = at + e - W if b else e
        I[b] = at
        if (e > R) if b else (at > (T // CHUNK) * CHUNK):
            return NO_ROOM, tuple(I), b + 1
    if I[2] > T:
        return BAD_COUNT, tuple(I), 4
    j_end = T - I[2] + W
    if j_end > R:
        return NO_ROOM, tuple(I), 4
    c, q, st = P.snap[3]
    js = c * CHUNK
    if j_end > js:
        # the over-read rule at the stream's last symbol (bitreader.go:113-120), on part 3's own count, from its last chunk start
        # with bits left; more than a chunk behind it: the chunk behind the snapshot started without bits
        if j_end - js > CHUNK or s.run(q, list(st), js, j_end - js) < 0:
            return BAD_COUNT, tuple(I), 4
    return DONE, tuple(I), 0


def joined(s, W=OVERLAP):
    """the states k_dec_translate reads of a DONE unit: tok[i] below I_1, then part p's steps W + i - I_p"""
    P = Parts(s, W, keep=True)
    outcome, I, _ = split4(s, W, parts=P)
    assert outcome == DONE, outcome
    bounds = [0, *I, s.count]
    out = list(P.steps[0][:I[0]])
    for p in range(1, PARTS):
        n = bounds[p + 1] - bounds[p]
        seg = P.steps[p][P.W:P.W + n]
        assert len(seg) == n, (p, len(seg), n)
        out += seg
    return out, I
