"""A plain numpy restatement of the tANS encode stage (csrc/mic_encode.hip: te_small_class, the gates of k_enc_tans_wg, te_encode and
the trailer of te_pack), written from the kernel's own account of itself and the reference lines it cites
(fsecompressu16.go:95-100, fse2state.go:122-199, ransu16.go:187-197, bitwriter.go).

    classify        which k_enc_tans_wg instance takes a unit (MicUnit.enc_kernel), its thread count and whether the coding records
                    sit in LDS
    te_encode       the partition (nblk, per, lastown), the warm-up, the speculative walk with one record per 128 tokens, the fix-up
                    rounds to the fixed point as the kernel runs them (MicUnit.enc_rounds), every thread's bits, the bitstream
    encode          the attempts of one unit: length gates, size verdict, the fallback chain, the two-state instance's hand-over

The walk is vectorised over the group's threads and serial along a thread's tokens, as the device is.  Nothing here imports the
package under test; tests/test_tans_encode_cpu.py holds the bitstream against the oracle byte for byte, case by case."""
from collections import namedtuple

import numpy as np

import table_routes as M

NARROW2, WIDE, SMALL12, SMALL13, TL14, TL15, TL16, SERIAL = 1, 2, 3, 4, 5, 6, 7, 8   # MicUnit.enc_kernel: 1 + bit index of MIC_ENC_CLS_*
KERNELS = {NARROW2: "narrow2", WIDE: "wide", SMALL12: "small12", SMALL13: "small13", TL14: "tl14", TL15: "tl15", TL16: "tl16", SERIAL: "serial"}
SMALL_NTOK, SMALL_SYMS, TT_SYMS = 98304, 1024, 4096                        # TE_SMALL_NTOK, TE_SMALL_SYMS, TE_TT_SYMS
WARM_TOK, REC_TOK = 128, 128                                               # TE_WARM_TOK; tokens per fix-up record (RGRP blocks)
STAGING_ALIGN = 256                                                        # bytes a unit's staging blob is aligned to (mic_session.h: blob_s, which points back here)
ERR_INTERNAL, ERR_INCOMPRESSIBLE = M.ERR_INTERNAL, M.ERR_INCOMPRESSIBLE

Cls = namedtuple("Cls", "kernel T ttl")


def classify(ntok, tl, symbol_len, flavour, handed=False):
    """the instance whose gates (tl_lo / tl_hi, te_small_class, WIDTH) match the unit"""
    if tl == 14:
        return Cls(TL14, 512, symbol_len <= TT_SYMS)
    if tl == 15:
        return Cls(TL15, 512, symbol_len <= TT_SYMS)
    if tl == 16:
        return Cls(TL16, 1024, False)
    if ntok <= SMALL_NTOK and symbol_len <= SMALL_SYMS:                    # te_small_class: the one-wave instances
        return Cls(SMALL12 if tl <= 12 and symbol_len <= 512 else SMALL13, 64, True)
    if flavour == 2 and symbol_len <= TT_SYMS and not handed:
        return Cls(NARROW2, 512, True)
    return Cls(WIDE, 512, symbol_len <= TT_SYMS)


def blk_of(lanes, rans, ttl):
    return 64 if lanes == 2 and not rans and ttl else 32


Walk = namedtuple("Walk", "N BLK T nblk per lastown gper rounds mybits zero_threads sym_bits total_bytes bits fin")


class _Stepper:
    """one coding step for a vector of (state, symbol) pairs -> (new state, bits emitted); states are whole (2^tl .. 2^(tl+1))"""

    def __init__(self, norm, tl, rans):
        self.size, self.rans = 1 << tl, rans
        if rans:
            nb, find = M.rans_ctable(norm, tl)
        else:
            st, nb, find, _ = M.ctable(norm, tl)
            self.state_tab = st.astype(np.int64)
        self.nb, self.find = nb.astype(np.int64), find.astype(np.int64)

    def __call__(self, state, sy):
        if self.rans:
            e = self.nb[sy]
            freq, k0 = e & 0xFFFFF, e >> 20
            k = k0 - (state < (freq << k0))
            return self.size + self.find[sy] + ((state >> k) - freq), k
        nb = ((state + self.nb[sy]) & 0xFFFFFFFF) >> 16
        return self.state_tab[(state >> nb) + self.find[sy]], nb

    def scalar(self):
        """the same step on plain integers (one thread re-walking alone, round after round, is most of a long fix-up)"""
        nbl, findl, size = self.nb.tolist(), self.find.tolist(), self.size
        if self.rans:
            def one(state, sy):
                e = nbl[sy]
                freq, k0 = e & 0xFFFFF, e >> 20
                k = k0 - (state < (freq << k0))
                return size + findl[sy] + ((state >> k) - freq), k
        else:
            tab = self.state_tab.tolist()

            def one(state, sy):
                nb = ((state + nbl[sy]) & 0xFFFFFFFF) >> 16
                return tab[(state >> nb) + findl[sy]], nb
        return one


def te_encode(sym, norm, tl, lanes, rans, T, ttl, want_bits=True):
    """te_encode<N, RANS, TTL, T> on the tokens `sym` -> Walk"""
    N = 8 if rans else lanes
    BLK = blk_of(N, rans, ttl)
    n, size = int(sym.size), 1 << tl
    step = _Stepper(norm, tl, rans)
    sym = np.asarray(sym, np.int64)
    nblk = (n + BLK - 1) // BLK
    per = (nblk + T - 1) // T
    lastown = (nblk + per - 1) // per
    tid = np.arange(T)
    b_hi = np.where(tid * per < nblk, nblk - tid * per, 0)
    b_lo = np.where(b_hi > per, b_hi - per, 0)
    top, L = b_hi * BLK, (b_hi - b_lo) * BLK                               # a thread walks tokens top - 1 .. top - L, downwards
    gper = (per * BLK + REC_TOK - 1) // REC_TOK
    own = L > 0
    plain = []

    def walk(rows, st, s_lo, s_hi, out=None):
        """tokens top - 1 - s for s in [s_lo, s_hi) of threads `rows`, states st[len(rows), N] in place -> bits per thread"""
        bits = np.zeros(rows.size, np.int64)
        if out is None and rows.size <= 48:
            if not plain:
                plain.extend([step.scalar(), sym.tolist()])
            one, syml = plain
            for r, t in enumerate(rows.tolist()):
                cur, tp = st[r].tolist(), int(top[t])
                for s in range(s_lo, min(s_hi, int(L[t]))):
                    if tp - 1 - s < n:
                        k = (-1 - s) % N
                        cur[k], nb = one(cur[k], syml[tp - 1 - s])
                        bits[r] += nb
                st[r] = cur
            return bits
        for s in range(s_lo, s_hi):
            idx = top[rows] - 1 - s
            act = (s < L[rows]) & (idx < n)
            if not act.any():
                continue
            k = (-1 - s) % N                                               # top is a multiple of BLK, so of N: the chain of token idx
            a = np.flatnonzero(act)
            state = st[a, k]
            new, nb = step(state, sym[idx[a]])
            st[a, k] = new
            bits[a] += nb
            if out is not None:
                out[0][rows[a], s] = state & ((1 << nb) - 1)
                out[1][rows[a], s] = nb
        return bits

    # ---- 1. warm-up and speculative walk ----------------------------------------------------------------------------------------
    st = np.full((T, N), size, np.int64)
    warm = np.flatnonzero(own & (tid > 0))
    if warm.size:
        w_top = np.minimum(np.minimum(b_hi[warm] + WARM_TOK // BLK, nblk) * BLK, n)      # w_hi = min(b_hi + WARM, nblk), bounded last block
        for s in range(int((w_top - top[warm]).max())):                    # every thread downwards from its own w_top, nothing recorded
            idx = w_top - 1 - s
            a = np.flatnonzero(idx >= top[warm])
            chain = idx[a] % N                                             # (w_top is n for the threads the stream's end clips)
            for k in np.unique(chain):
                b = a[chain == k]
                st[warm[b], k] = step(st[warm[b], k], sym[idx[b]])[0]
    assumed = st.copy()
    rec_st = np.zeros((T, gper, N), np.int64)
    rec_bits = np.zeros((T, gper), np.int64)
    mybits = np.zeros(T, np.int64)
    rows_all = np.flatnonzero(own)
    for g in range(gper):
        rows = rows_all[L[rows_all] > g * REC_TOK]
        if not rows.size:
            break
        cur = st[rows]
        bits = walk(rows, cur, g * REC_TOK, (g + 1) * REC_TOK)
        st[rows] = cur
        mybits[rows] += bits
        rec_st[rows, g], rec_bits[rows, g] = cur, bits
    E = st.copy()
    # ---- 2. fix-up rounds to the fixed point ------------------------------------------------------------------------------------
    rounds = 0
    for _ in range(T):
        rounds += 1
        e_prev = np.vstack([np.full((1, N), size, np.int64), E[:-1]])
        anyd = (e_prev != assumed).any(axis=1) & (tid > 0)
        assumed = np.where((tid > 0)[:, None], e_prev, assumed)
        e_out = E.copy()
        changed = False
        active = np.flatnonzero(anyd & own)
        st2 = e_prev[active].copy()
        for g in range(gper):
            keep = L[active] > g * REC_TOK
            done = active[~keep]                                           # ran to the end of the range unmerged: hand the states on
            if done.size:
                d2 = st2[~keep]
                changed |= bool((d2 != e_out[done]).any())
                e_out[done] = d2
            active, st2 = active[keep], st2[keep]
            if not active.size:
                break
            bits = walk(active, st2, g * REC_TOK, (g + 1) * REC_TOK)
            merged = (rec_st[active, g] == st2).all(axis=1)
            mybits[active] += bits - rec_bits[active, g]
            rec_st[active, g], rec_bits[active, g] = st2, bits
            active, st2 = active[~merged], st2[~merged]
        if active.size:                                                    # unmerged behind the last record
            changed |= bool((st2 != e_out[active]).any())
            e_out[active] = st2
        E = e_out
        if not changed:
            break
    # ---- 3. bit offsets, 4. pack from the true start states ------------------------------------------------------------------------
    fin = E[lastown - 1].copy()
    sym_bits = int(mybits.sum())
    total_bits = sym_bits + N * tl + 1
    total_bytes = (total_bits + 7) >> 3
    zero_threads = frozenset(int(t) for t in np.flatnonzero(own & (mybits == 0)))
    bits = None
    if want_bits:
        stp = np.vstack([np.full((1, N), size, np.int64), E[:-1]])
        stp[lastown:] = size
        val, nbm = np.zeros((T, gper * REC_TOK), np.int64), np.zeros((T, gper * REC_TOK), np.int64)
        cur = stp[rows_all].copy()
        packed = walk(rows_all, cur, 0, int(L.max()), out=(val, nbm))
        assert np.array_equal(packed, mybits[rows_all]), "the records' bit counts are not those of the walk from the true states"
        assert rows_all[-1] == lastown - 1 and np.array_equal(cur[-1], fin), "the last owner's end states are not the final states"
        v, b = val.ravel(), nbm.ravel()                                    # thread by thread, each downwards: the emission order
        v, b = v[b > 0], b[b > 0]
        v = np.concatenate([v] + [[int(fin[k]) & (size - 1)] for k in range(N - 1, -1, -1)] + [[1]])   # final states, last lane first; end mark
        b = np.concatenate([b, np.full(N, tl, np.int64), [1]])
        off = np.cumsum(b) - b
        assert int(b.sum()) == total_bits
        stream = np.zeros(total_bytes * 8, np.uint8)
        for j in range(17):
            m = b > j
            if not m.any():
                break
            stream[off[m] + j] = (v[m] >> j) & 1
        bits = np.packbits(stream, bitorder="little").tobytes()
    return Walk(N, BLK, T, nblk, per, lastown, gper, rounds, mybits, zero_threads, sym_bits, total_bytes, bits, fin)


Result = namedtuple("Result", "status flavour kernel handed rounds walk blob attempts")


def _prefix(lanes, rans, n):
    if lanes == 1:
        return b""
    return bytes([0xFF, 0x08 if rans else {2: 0x02, 4: 0x04, 8: 0x84}[lanes]]) + int(n).to_bytes(4, "little")


def encode(sym, u, flavour, chain=False, want_bits=True):
    """the tANS stage of one unit whose table stage `u` (table_routes.Unit) succeeded: every attempt k_enc_tans_wg makes.
    chain: no_fallback = 0 (flavour -> flavour / 2 -> ... -> 1 over the one table, a failed two-state attempt of the narrow
    instance handed to the wide one, which starts over); else the one attempt of a bare FSECompressU16* call."""
    assert u.rc == 0
    n, rans = int(sym.size), flavour == 108
    assert not (rans and chain)
    handed = False
    cls = classify(n, u.tl, u.symbol_len, flavour)
    attempts = []
    lanes = 8 if rans else flavour
    while True:
        rc, w = 0, None
        if n <= lanes - 1 or n <= 1:
            rc = ERR_INCOMPRESSIBLE
        elif n <= 2 and lanes <= 2:
            rc = ERR_INTERNAL
        else:
            w = te_encode(sym, u.norm, u.tl, lanes, rans, cls.T, cls.ttl, want_bits)
            if u.hdr_len + w.total_bytes >= 2 * n:                         # fse2state.go:58-60
                rc = ERR_INCOMPRESSIBLE
        attempts.append((cls.kernel, lanes, rc))
        if rc == 0:
            blob = _prefix(lanes, rans, n) + bytes(u.header) + w.bits if want_bits else None
            return Result(0, lanes, cls.kernel, handed, w.rounds, w, blob, attempts)
        if lanes == 1 or not chain:
            return Result(rc, 0, cls.kernel, handed, w.rounds if w else 0, w, b"", attempts)
        if cls.kernel == NARROW2:                                          # nstates_used = -2: the wide instance starts over
            handed, cls = True, classify(n, u.tl, u.symbol_len, flavour, handed=True)
            lanes = flavour
            continue
        lanes >>= 1
