"""CPU model of the eight-part instance of the split two-state tANS decode (csrc/mic_decode_ls.hip: k_dec_tans_ls_parts<8>; DESIGN.md
section 4), on top of tests/tans_split_model.py, which is generic in the number of parts (a chunk is 128 / n = 16 symbols).

What the eight-part instance does differently, and only that, is stated here:
  * a scratch region holds a part's steps from W on (step j >= W at region offset j - W), so the room rules are e_p - W <= R at a
    middle boundary and j_end - W <= R at the stream's end -- the four-part model's rules with R + W in R's place;
  * R is a seventh of the unit's token slab in whole chunks;
  * a class-0 unit of at least max(min_tokens8, min_tokens4) tokens takes the eight-part list, and what the instance hands back
    the four-part instance judges afresh: `outcome` is the record such a unit ends up with."""
import tans_split_model as M

N = 8
CHUNK = 128 // N
MIN_TOKENS8 = 393216                                            # MicSplitCfg::min_tokens8
EIGHT_PARTS = "split8"


def region(px):
    """R of a tier-1 eight-part unit of `px` pixels: a seventh of its token slab, in whole chunks"""
    return ((px + px // 8 + 4096) // 7) & ~(CHUNK - 1)


def split8(s, W=M.OVERLAP, R=None, parts=None):
    """(outcome, (I_1 .. I_7), failing boundary) of the eight-part kernel for overlap W and regions of R tokens (default: enough)"""
    return M.split_parts(s, W, R=None if R is None else R + (W & ~63), parts=parts, n=N)


def route(s, min_tokens=M.MIN_TOKENS, min_tokens4=M.MIN_TOKENS4, min_tokens8=MIN_TOKENS8, min_bits16=M.MIN_BITS16):
    r = M.route(s, min_tokens=min_tokens, min_tokens4=min_tokens4, min_bits16=min_bits16)
    return EIGHT_PARTS if r == M.FOUR_PARTS and s.count >= max(min_tokens8, min_tokens4) else r


def joined(s, W=M.OVERLAP):
    """the states k_dec_translate reads of a DONE unit: tok[i] below I_1, then sym[(p - 1) R + i - I_p], which is part p's step
    W + i - I_p"""
    return M.joined(s, W, n=N)


def outcome(s, W, R8, R4):
    """the record an eight-part unit ends up with -> (parts, outcome, I, failing boundary): the eight-part instance's when it joins,
    else the four-part instance's, which takes the unit from the end of its list"""
    o, I, f = split8(s, W, R=R8)
    if o == M.DONE:
        return N, o, I, f
    o, I, f = M.split_parts(s, W, R=R4, n=4)
    return 4, o, I, f
