"""CPU model of the two-chunk pass of the eight-part split decode (csrc/mic_decode_ls.hip: k_dec_tans_ls_parts<8>, the chain wave's
loop and the partner's register queue; DESIGN.md section 4, "Partner waves"), on top of tests/tans_partner_model.py and
tests/tans_split8_model.py, which it imports and does not change.

What the pass changes, and only that, is stated here:
  * a pass of the chain wave's loop is an even chunk and an odd one, and the wave-uniform exit test stands in front of the even one
    only: a wave whose last part goes off in front of an odd chunk runs that chunk all the same (`chunks_pass`).  Nothing is on in
    it, so no record moves; what it does is a chunk's reads, a chunk's publish and a chunk's state stores (`extra_chunk_stores`);
  * the partner keeps the two blocks under the ring in two registers named by the block's parity, loads both again every chunk, and
    waits, in front of a chunk's fills, for the loads of two chunks ago and older only (`QueuePart`).  A block enters the queue at
    one advance of its part and the ring at the next but one, and a part advances once a chunk at the most.

`check` plays PM.schedule's two extreme service schedules over chunks_run + 1 chunks -- the most a unit's own wave adds to it -- with
the queue in place of PM.Part's plain fill."""
import tans_partner_model as PM
import tans_split_model as M
import tans_split8_model as M8

CHUNK = PM.CHUNK
LOAD_LEAD = 2                                                   # chunks between a load and the wait that covers it (s_waitcnt vmcnt(24))


def chunks_pass(n):
    """chunks a chain wave runs whose parts are on for chunks 0 .. n - 1: the loop as the kernel has it"""
    c = 0
    while True:
        if c >= n:                                                          # the exit test: in front of the pass's first chunk
            return c
        c += 2                                                              # the even chunk, then the odd one


class QueuePart(PM.Part):
    """PM.Part with the partner's two registers: reg[parity] = (block, chunk whose service first issued its load; None: the kernel's start)"""

    def __init__(self, rows, ring_only=False):
        super().__init__(rows, ring_only)
        self.reg = {b & 1: (b, None) for b in (self.next, self.next - 1)}
        self.lead = []                                                      # chunks between a block's first load and its fill

    def serve(self, c):
        fills, nxt = len(self.filled), self.next
        super().serve(c)
        if len(self.filled) > fills:                                        # the part has reached a new block: the ring took block nxt
            b, issued = self.reg[nxt & 1]
            assert b == nxt, ("chunk %d: the register of parity %d holds block %d, the ring takes %d" % (c, nxt & 1, b, nxt))
            assert issued is None or issued <= c - LOAD_LEAD, ("chunk %d: block %d was loaded in chunk %d, the wait covers chunk %d" % (c, b, issued, c - LOAD_LEAD))
            if issued is not None:
                self.lead.append(c - issued)
        for b in (self.next, self.next - 1):                                # both blocks again; one that is there keeps its first load
            if self.reg[b & 1][0] != b:
                self.reg[b & 1] = (b, c)
        assert {v[0] for v in self.reg.values()} == {self.next, self.next - 1}


def check(s, W, sb=0, lag=0, parts=None, ring_only=False, extra=1):
    """PM.check over chunks_run + extra chunks, with the register queue -> (chunks played, fills per part, the shortest lead of a load)"""
    n = PM.chunks_run(s, W, parts) + extra
    pos = PM.positions(s, W, sb, n)
    fills, lead = [], []
    for late in (False, True):
        for p, rows in enumerate(pos):
            part = QueuePart(rows, ring_only)
            for what, c in PM.schedule(n, late, lag):
                try:
                    getattr(part, what)(c)
                except AssertionError as e:
                    raise AssertionError("part %d, %s schedule, lag %d: %s" % (p, "late" if late else "early", lag, e)) from None
            if late:
                fills.append(len(part.filled))
                for c, placed, gone in part.filled:
                    assert all(gone not in PM.reads(rows[k]) for k in range(c + 1, min(c + 4, n))), (p, c, placed, gone)
            lead += part.lead
    return n, fills, min(lead)


def extra_chunk_stores(T, W, R, c):
    """where the state stores of chunk c land, per part: ("tok" | region index, first token offset), or None for a store the kernel
    drops -- part 0 writes tok, whose descriptor ends at the stream's last whole chunk; part p >= 1 writes region p - 1 from step W
    on (step j at offset j - W) when the chunk lies behind the overlap and inside the region (`fits`)"""
    wc = (W & ~63) // CHUNK
    out = [("tok", c * CHUNK) if (c + 1) * CHUNK <= (T // CHUNK) * CHUNK else None]
    for p in range(1, M8.N):
        out.append((p - 1, (c - wc) * CHUNK) if c >= wc and (c + 1 - wc) * CHUNK <= R else None)
    return out


def live(T, W, I):
    """tokens of each slab that k_dec_translate reads of a DONE unit with boundaries I: tok [0, I_1), region p - 1 [0, I_p+1 - I_p)"""
    bounds = [0, *I, T]
    return {"tok": bounds[1], **{p - 1: bounds[p + 1] - bounds[p] for p in range(1, M8.N)}}
