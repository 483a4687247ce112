"""The two-chunk pass of the eight-part split decode (tests/tans_pairs_model.py) on the oracle's own streams, the three that
tests/test_tans_partner_cpu.py uses: the 9.57-bit strip, the fastest consumer found (11.66 bits per token) and the falling-noise strip,
at each of the four byte offsets a bitstream can have against the dword grid.  No GPU.

With the exit test in front of even chunks only a chain wave runs one chunk more than its parts need when that count is odd.  Checked
here, over chunks_run + 1 chunks whatever the parity: both extreme service schedules still find every block a chunk reads and never
write a stage or mailbox half that is not taken; one chunk later than the rule it still fails; the partner's register queue holds the
block the ring takes, loaded two chunks before at the least; and the chunk behind a unit's last own chunk stores nothing where anything
is read.

About that last point.  Part 0's chunk behind the last own one lies at token 16 chunks_run, inside tok's whole chunks for every unit
that joins (the parts end near T / 8 + W), and a middle part's lies inside its region: the place a shorter stream's chunks have always
gone to beside a longer neighbour.  What holds, and what the pixels need, is that it lies behind the last token k_dec_translate reads
of that slab (tok below I_1, region p - 1 below I_p+1 - I_p), or is dropped by the descriptor or by `fits`.  Outside tok's whole chunks
and outside R it lies for the unit that runs to the cap."""
import pytest

import tans_pairs_model as PP
import tans_partner_model as PM
import tans_split_model as M
import tans_split8_model as M8
import test_tans_partner_cpu as TP

W = TP.W
NAMES = ["published", "fast", "falling"]


def test_the_exit_test_of_a_pass():
    assert [PP.chunks_pass(n) for n in range(6)] == [0, 2, 2, 4, 4, 6]
    assert all(n <= PP.chunks_pass(n) <= n + 1 and PP.chunks_pass(n) % 2 == 0 for n in range(200))


@pytest.mark.parametrize("name", NAMES)
def test_the_deadline_holds_over_one_chunk_more(mico, synth, name):
    s, P = TP._stream(mico, synth, name)
    assert M8.split8(s, W, parts=P)[0] == M.DONE
    n0 = PM.chunks_run(s, W, P)
    for sb in range(4):
        n, fills, lead = PP.check(s, W, sb=sb, parts=P)
        assert n == n0 + 1 >= PP.chunks_pass(n0) and all(f > 0 for f in fills)
        assert lead >= PP.LOAD_LEAD, lead                                   # a block is in its register before its fill is due
        if sb == 0:
            assert PP.check(s, W, sb=0, parts=P, extra=0)[0] == n0              # (and over the unit's own chunks, the queue in place)


def test_a_partner_one_chunk_later_is_still_too_late(mico, synth):
    s, P = TP._stream(mico, synth, "fast")
    with pytest.raises(AssertionError, match="late schedule, lag 1"):
        PP.check(s, W, sb=0, lag=1, parts=P)
    for name in ("fast", "published"):
        s, P = TP._stream(mico, synth, name)
        with pytest.raises(AssertionError, match="late schedule, lag 1: chunk [0-9]+ reads block"):
            PP.check(s, W, sb=0, lag=1, parts=P, ring_only=True)
        PP.check(s, W, sb=0, lag=0, parts=P, ring_only=True)


def test_a_load_one_chunk_ahead_would_not_do(mico, synth, monkeypatch):
    """the fastest consumer advances in consecutive chunks, so a wait that covered the chunk before as well is what the two-register
    queue with a moved register needed; with the parity registers a block's load is two advances old when the ring takes it"""
    s, P = TP._stream(mico, synth, "fast")
    monkeypatch.setattr(PP, "LOAD_LEAD", 3)
    with pytest.raises(AssertionError, match="was loaded in chunk"):
        PP.check(s, W, sb=0, parts=P)


@pytest.mark.parametrize("name", NAMES)
def test_the_chunk_behind_the_last_own_one_stores_nothing_that_is_read(mico, synth, name):
    s, P = TP._stream(mico, synth, name)
    o, I, _ = M8.split8(s, W, parts=P)
    assert o == M.DONE
    T, n = s.count, PM.chunks_run(s, W, P)
    R = M8.region(2577 * (64 if name == "falling" else 48))
    live = PP.live(T, W, I)
    for c in (n, n + 1):                                                    # the chunk a pass adds to an odd count, and to an even one beside a neighbour
        stores = PP.extra_chunk_stores(T, W, R, c)
        assert len(stores) == 8 and any(x is not None for x in stores)
        for x in stores:
            assert x is None or x[1] >= live[x[0]], (c, x, live)
        assert all(x is None or x[1] + PP.CHUNK <= (T if x[0] == "tok" else R) for x in stores)


def test_a_unit_that_runs_to_the_cap_stores_outside_tok_and_its_regions(mico, synth):
    """no hand-over inside the unit's chunks (W beyond its length): every part runs to the cap, count // 16 + 2, and the chunk behind
    it falls outside tok's whole chunks and in front of every region's first step (regions hold steps from W on)"""
    s, _ = TP._stream(mico, synth, "published")
    Wbig = 131072
    P = M.Parts(s, Wbig, n=8)
    assert not P.handed
    n = PM.chunks_run(s, Wbig, P)
    assert n == s.count // 16 + 2
    R = M8.region(2577 * 48)
    for c in (n, n + 1):
        assert PP.extra_chunk_stores(s.count, Wbig, R, c) == [None] * 8
    assert PP.extra_chunk_stores(s.count, Wbig, R, s.count // 16 - 1)[0] == ("tok", (s.count // 16 - 1) * 16)   # (the last whole chunk is stored)
