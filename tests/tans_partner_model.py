"""CPU model of the partner protocol of the eight-part split decode (csrc/mic_decode_ls.hip: k_dec_tans_ls_parts<8>, the comment above
the kernel), on top of tests/tans_split_model.py.

A plain-Python restatement of the schedule of one part of one stream: its chunk loop (16 symbols a chunk, eight rounds of two), the
ring of four blocks of eight dwords it reads its bit window from, the two stage halves and the two mailbox halves, by chunk parity,
and the partner wave that serves chunk c behind the chain wave -- it reads the position published behind chunk c, puts block b - 2
into the ring when the position has reached a new block b, and sends stage half c & 1 out.  The one rule that couples the two is the
kernel's: the chain wave starts chunk c only when chunks 0 .. c - 2 are served.

Positions are counts of unread bits as in tans_split_model, moved onto the kernel's grid of aligned dwords: P = p + 8 sb for a
stream whose first byte lies sb bytes behind a dword boundary.  The kernel tracks q = P - 32; a block is (q >> 5) >> 3.
Reads, as stated above LsParts: for every position P of a chunk, its last included, the three dwords from the dword of P - 64 on.

`check` plays the two extreme schedules the rule allows -- the partner serves chunk c at once, or only when the chain wave is about
to start chunk c + 2 -- and asserts in both that every dword a chunk reads is in the ring, that no stage half and no mailbox half is
written before the partner has taken it, and that the partner finds what it comes for.  A fill stores one block, so any timing in
between is one of the two for every single read.  `lag` = 1 lets the partner serve a chunk later than the rule allows: the test
shows that this fails, so the deadline is the rule's and not a chunk looser."""
import tans_split_model as M

N = 8
CHUNK = 128 // N                                                # symbols of a chunk of one part
ROUNDS = CHUNK // 2
BLK = 64 // N                                                   # dwords of a ring block
SLOTS, DEPTH = 4, 2                                             # LsParts::RING_BLOCKS, DEPTH


def chunks_run(s, W, parts=None):
    """chunks the unit's own parts run: the last chunk any part is on for, + 1 (MicUnit.partner[1] of a unit its partner served whole)"""
    P = parts or M.Parts(s, W, n=N)
    if not P.handed:
        return s.count // CHUNK + 2                                         # no hand-over inside the unit's chunks: every part runs to the cap
    return max(sn[0] for sn in P.snap) + 1


def positions(s, W, sb, n_chunks):
    """per part, per chunk, the grid positions at the start of every round and behind the last: ROUNDS + 1 values.  Every part runs
    all n_chunks, on or not (a part that is off runs on into its lower neighbour's bits, the last part into zeros)"""
    out = []
    for p, start in enumerate(M.starts(s, W & ~63, N)):
        q, a, b = s.start(start)
        st, i, per = [a, b], 0, []
        for _ in range(n_chunks):
            row = [q + 8 * sb]
            for _ in range(ROUNDS):
                q = s.run(q, st, i, 2)
                i += 2
                row.append(q + 8 * sb)
            per.append(row)
        out.append(per)
    return out


def block(P):
    return ((P - 32) >> 5) >> 3


def reads(row):
    """blocks of the dwords a chunk with the round positions `row` reads"""
    return {(((P - 64) >> 5) + k) >> 3 for P in row for k in range(3)}


def schedule(n, late, lag=0):
    """the events of one part: ("run", c) and ("serve", c).  late: chunk c is served when the chain wave is about to start chunk
    c + 2 + lag (lag 0: the last moment the kernel's rule allows); else right behind the chunk"""
    ev = []
    for c in range(n):
        if late and c - 2 - lag >= 0:
            ev.append(("serve", c - 2 - lag))
        ev.append(("run", c))
        if not late:
            ev.append(("serve", c))
    if late:
        ev += [("serve", c) for c in range(max(n - 2 - lag, 0), n)]
    return ev


class Part:
    """ring, stage halves and mailbox halves of one part"""

    def __init__(self, rows, ring_only=False):
        self.rows, self.ring_only = rows, ring_only                         # ring_only: the halves are not modelled (every chunk keeps its own)
        b = block(rows[0][0])
        self.ring = {(b - d) % SLOTS: b - d for d in range(-1, DEPTH + 1)}   # the chain wave's start: blocks b + 1 .. b - 2
        self.next = b - DEPTH - 1                                           # the block the partner's queue holds first
        self.stage, self.mail = [None, None], [None, None]                  # chunk held, or None once the partner has taken it
        self.filled = []                                                    # (chunk served, block placed, block it replaced)

    def run(self, c):
        row = self.rows[c]
        for b in reads(row):
            assert self.ring[b % SLOTS] == b, ("chunk %d reads block %d, slot holds %d" % (c, b, self.ring[b % SLOTS]))
        h = c if self.ring_only else c & 1
        if self.ring_only:
            self.stage[h:h + 1], self.mail[h:h + 1] = [None], [None]
        assert self.stage[h] is None, ("chunk %d writes stage half %d over chunk %d's states" % (c, h, self.stage[h]))
        assert self.mail[h] is None, ("chunk %d writes mailbox half %d over chunk %d's position" % (c, h, self.mail[h]))
        self.stage[h], self.mail[h] = c, (c, row[-1])

    def serve(self, c):
        h = c if self.ring_only else c & 1
        assert self.mail[h] is not None and self.mail[h][0] == c and self.stage[h] == c, (c, self.mail[h], self.stage[h])
        b = block(self.mail[h][1])
        if b - DEPTH <= self.next:                                          # the part has reached a new block: one at most per chunk
            assert b - DEPTH == self.next, ("chunk %d: two blocks in one chunk (block %d, queue at %d)" % (c, b, self.next))
            self.filled.append((c, self.next, self.ring[self.next % SLOTS]))
            self.ring[self.next % SLOTS] = self.next
            self.next -= 1
        self.stage[h] = self.mail[h] = None


def check(s, W, sb=0, lag=0, parts=None, ring_only=False):
    """plays both schedules for every part of the stream -> (chunks, fills per part, the most dwords a chunk moved)"""
    n = chunks_run(s, W, parts)
    pos = positions(s, W, sb, n)
    fills, most = [], 0
    for late in (False, True):
        for p, rows in enumerate(pos):
            part = Part(rows, ring_only)
            for what, c in schedule(n, late, lag):
                try:
                    getattr(part, what)(c)
                except AssertionError as e:
                    raise AssertionError("part %d, %s schedule, lag %d: %s" % (p, "late" if late else "early", lag, e)) from None
            if late:
                fills.append(len(part.filled))
                # no fill replaced a block that a chunk from the one behind the served chunk on reads
                for c, placed, gone in part.filled:
                    assert all(gone not in reads(rows[k]) for k in range(c + 1, min(c + 4, n))), (p, c, placed, gone)
            most = max(most, max((r[0] - r[-1]) for r in rows))
    return n, fills, most / 32.0
