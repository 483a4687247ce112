"""What can be said without a device about the cases of tests/test_gpu_table_routes.py: for every case of tests/table_streams.py the
plain-integer model of tests/table_routes.py agrees with the oracle on the gates, the tableLog, all 65536 normalised counts and the
header byte for byte; the oracle decodes its own blob; and the seam the case is named for -- a zero run over a tile border, a header
of 8177 bytes, 481 symbols of more than sixteen slots -- is worked out from the model and asserted, so a case cannot silently stop
aiming at it.  The union of the routes the model names covers every MIC_TBR_* bit of csrc/mic_dev.h.

`distributed == symbolLen + 1` (fsecompressu16.go, normalizeCount2) is unreachable -- at most symbolLen symbols are distributed --
and the model asserts that instead of a case for it."""
import os
import re

import numpy as np
import pytest

import table_routes as M
import table_streams as S
from conftest import ROOT

CASES = S.cases()
TILE = S.TILE

# every seam the issue lists must keep a case: the whole aim tuple, so that no two listed seams share a key
REQUIRED = {("norm", "PRIMARY"), ("norm", "N2_PAR"), ("norm", "N2_UNIFORM"), ("norm", "N2_SERIAL"), ("rc", M.ERR_INTERNAL),
            ("run", 1023, 1024), ("run", 1000, 2100), ("run", 383, 384),
            ("tile-runs", S.RUNS_A), ("tile-runs", S.RUNS_B), ("tile-runs", S.RUNS_A + S.RUNS_B),
            ("three-words",), ("last-bit", 0), ("last-bit", 1), ("wrap", False), ("wrap", True),
            ("scratch", 8192, 13, "SMALL"), ("scratch", 8193, 13, "HBM"), ("scratch", 9001, 10, "HBM"), ("scratch", 600, 13, "SMALL"),
            ("scratch", 600, 14, "HBM"), ("scratch", 9001, 15, "HBM"), ("scratch", 65536, 16, "HBM"),
            ("spread", 5, "low"), ("spread", 5, "nolow"), ("slots", (1, 2, 16, 17, 64, 65)), ("nbig", 13, 40), ("nbig", 13, 481),
            ("nbig-hbm", 14), ("nbig-hbm", 16),
            ("straddle", 8177, "P_SMALL"), ("straddle", 8178, "P_DEFER_LEN"), ("big", "P_BIG_STAGE"), ("big", "P_BIG_HBM"),
            ("defer", "P_DEFER_SYMS"), ("tail", "no-window"), ("tail", "inside-16+bail"), ("tail", "exactly-16"),
            ("rc", 0), ("rc", M.ERR_USE_RLE), ("rc", M.ERR_INCOMPRESSIBLE)}
# and the gates, each between units that succeed: (flavour, n, max count) of the refused units of the `gates` group
GATES = {(2, 50, 50), (2, 50, 1), (2, 100000, 2), (2, 1, 1), (4, 3, 2), (8, 7, 4), (108, 7, 4), (2, 16384, 4)}


def test_the_route_bits_are_the_kernels():
    src = open(os.path.join(ROOT, "medical-image-codec_amd", "csrc", "mic_dev.h")).read()
    bits = {name: 1 << int(sh) for name, sh in re.findall(r"#define\s+MIC_TBR_(\w+)\s+\(1u << (\d+)\)", src)}
    assert bits == M.BIT
    tab = open(os.path.join(ROOT, "medical-image-codec_amd", "csrc", "mic_tables.hip")).read()
    par = open(os.path.join(ROOT, "medical-image-codec_amd", "csrc", "mic_tables_par.h")).read()
    assert (f"#define TB_SMALL_SYMS {M.SMALL_SYMS}" in tab and f"#define TB_SMALL_TL {M.SMALL_TL}" in tab and
            f"#define TP_SMALLV {M.SMALLV} " in par and "#define TP_THREADS 1024" in par)
    assert "BIG ? 40u * 1024u : 8u * 1024u" in tab and (M.STAGE_BIG, M.STAGE_SMALL) == (40 * 1024, 8 * 1024)


def test_every_listed_seam_keeps_a_case():
    have = {c.aim for c in CASES}
    assert REQUIRED == have, (REQUIRED - have, have - REQUIRED)
    assert any(S.unit(c).rc == M.ERR_INTERNAL for c in S.group("normaliser"))      # the -8 case of the normaliser group itself
    refused = {(c.flavour, int(c.hist.sum()), int(c.hist.max())) for c in S.group("gates") if S.unit(c).rc}
    assert refused == GATES, (GATES - refused, refused - GATES)
    for g in S.GROUPS:
        assert S.group(g), g
    # the spread cases: each in flavours 2 and 108, three of them in 1, 4 and 8 as well
    by_name = {}
    for c in S.group("spread"):
        by_name.setdefault(c.name.split("/")[0] + str(c.req_tl), set()).add(c.flavour)
    assert all({2, 108} <= f for f in by_name.values()), by_name
    assert sum(1 for f in by_name.values() if {1, 4, 8} <= f) >= 3
    # the gates lie between units that succeed
    rcs = [S.unit(c).rc for c in S.group("gates")]
    assert rcs[0] == 0 and rcs[-1] == 0 and all(a == 0 or b == 0 for a, b in zip(rcs, rcs[1:]))


def test_the_routes_cover_every_bit(mico):
    seen = set()
    for c in CASES:
        u = S.unit(c)
        rc, _, blob = S.reference(mico, c)
        seen |= M.names(u.enc_route())
        if rc == 0:
            seen |= M.names(u.dec_route(len(blob)))
    assert seen == set(M.BITS), set(M.BITS) - seen


def _zero_run(norm, first, close):
    return norm[first - 1] != 0 and norm[close] != 0 and not norm[first:close].any() and close > first


def _check_aim(c, u, blob):
    aim, f = c.aim, u.fields
    kind = aim[0]
    after = len(blob) - u.prefix if blob else 0
    dec = M.names(u.dec_route(len(blob))) if blob else set()
    if kind == "norm":
        assert aim[1] in u.norm_route, u.norm_route
        if aim[1] == "N2_SERIAL":                                           # every count 1, then round-robin to 2
            assert set(u.norm.tolist()) == {1, 2}
        if aim[1] != "PRIMARY":
            assert "PRIMARY" not in u.norm_route
    elif kind == "run":
        first, close = aim[1:]
        assert _zero_run(u.norm, first, close)
        k = int(np.flatnonzero(f.sym == close)[0])
        assert f.R[k] == close - first - 1
        if first == 1023:                                                   # first zero the last symbol of a tile, closed by the first of the next
            assert first % TILE == TILE - 1 and close == first + 1
        elif first == 1000:                                                 # a whole tile inside the run: carry_fz passes a tile with no first zero
            assert close // TILE - first // TILE == 2
        else:                                                               # lane 63 of a wave, lane 0 of the next, inside one tile
            assert first % 64 == 63 and close == first + 1 and close % TILE != 0
    elif kind == "tile-runs":
        got = set()
        for k, z in enumerate(aim[1]):
            t = (k + 1) * TILE
            assert _zero_run(u.norm, t - z, t), (k, z)
            R = int(f.R[int(np.flatnonzero(f.sym == t)[0])])
            assert R == z - 1
            got.add((R // 24, R % 24 % 3))
        assert {r for _, r in got} == {0, 1, 2} and len({q for q, _ in got}) >= 3
    elif kind == "three-words":
        last = f.start + f.ones - 1
        assert ((f.ones > 0) & (last // 32 - f.start // 32 >= 2)).any()
    elif kind == "last-bit":
        assert f.bits % 8 == aim[1]                                         # 0: the last field ends on bit 7 of a byte; 1: on bit 0
    elif kind == "wrap":
        assert u.tl == 16 and u.n > 1 << 18 and int(f.flen.max()) == 17 and u.wraps == aim[1]
        assert ("W_SERIAL" if aim[1] else "W_PAR") in M.names(u.enc_route())
    elif kind == "scratch":
        assert (u.symbol_len, u.tl, M.scratch(u.symbol_len, u.tl)) == aim[1:]
        if aim[1] in (8192, 8193):
            assert 32768 < u.n <= 65536
    elif kind == "spread":
        assert u.tl == aim[1] and (1 << u.tl) // 32 == 1 and bool((u.norm == -1).any()) == (aim[2] == "low")
    elif kind == "slots":
        assert set(aim[1]) <= set(u.norm.tolist())
    elif kind == "nbig":
        assert u.tl == aim[1] and M.nbig(u.norm, 2) == aim[2] > 16 and M.scratch(u.symbol_len, u.tl) == "SMALL"   # a second round for wave 0
        if aim[2] == 481:
            assert aim[2] == (1 << 13) // 17 and int(u.norm.min()) == 17       # the most the list can hold
    elif kind == "nbig-hbm":
        assert u.tl == aim[1] and M.nbig(u.norm, 2) >= 2 and M.scratch(u.symbol_len, u.tl) == "HBM"
        assert ((1 << u.tl) // 32 + 1023) // 1024 == (2 if aim[1] == 16 else 1)   # bitmap words in scan tiles of 1024
    elif kind == "straddle":
        assert u.hdr_len == aim[1] and len(blob) > M.STAGE_SMALL and u.symbol_len <= 8192 and u.tl == 13
        assert (u.hdr_len + 8 < M.STAGE_SMALL - u.prefix) == (aim[2] == "P_SMALL") and aim[2] in dec
    elif kind == "big":
        assert u.tl == 16 and len(blob) > M.STAGE_BIG and aim[1] in dec
        assert (u.hdr_len + 8 < M.STAGE_BIG - u.prefix) == (aim[1] == "P_BIG_STAGE")
    elif kind == "defer":
        assert aim[1] in dec and len(blob) <= M.STAGE_SMALL and u.tl <= 13 and u.symbol_len > 8192
    elif kind == "tail":
        lim = (after - 16) * 8
        if aim[1] == "no-window":
            assert after < 24 and "P_WINDOW" not in dec
        else:
            assert after >= 24 and "P_WINDOW" in dec
        if aim[1] == "inside-16+bail":
            assert 0 <= after - u.hdr_len < 16                             # the header ends inside the last sixteen bytes ...
            chunks = f.R // 24                                              # ... and a run's 16-bit chunks start inside the window's reach and leave it
            assert ((chunks > 0) & (f.start <= lim) & (f.start + 16 * chunks > lim)).any()
        elif aim[1] == "exactly-16":
            assert after - u.hdr_len == 16
    elif kind == "rc":
        assert u.rc == aim[1]
    else:
        raise AssertionError(("unknown aim", aim))


@pytest.mark.parametrize("group", S.GROUPS)
def test_the_model_is_the_oracle_and_every_case_reaches_its_seam(mico, group):
    for c in S.group(group):
        u = S.unit(c)
        rc, facts, blob = S.reference(mico, c)
        assert rc == u.rc, (c.name, rc, u.rc)
        if rc:
            _check_aim(c, u, b"")
            continue
        got = (facts["table_log"], facts["symbol_len"], facts["max_count"], facts["hdr_len"], facts["zero_bits"])
        assert got == (u.tl, u.symbol_len, u.max_count, u.prefix + u.hdr_len, u.dec_zero_bits), (c.name, got)
        norm = np.zeros(65536, np.int64); norm[:u.symbol_len] = u.norm
        assert np.array_equal(facts["norm"], norm), (c.name, np.flatnonzero(facts["norm"] != norm)[:4])
        head = blob[u.prefix:u.prefix + u.hdr_len]
        if head != u.header:
            i = next(i for i in range(u.hdr_len) if head[i] != u.header[i])
            raise AssertionError((c.name, "first differing header byte", i, head[i], u.header[i]))
        sym = S.symbols(c)
        rcd, back = mico.fse_decompress_auto(blob, sym.size + 8)
        assert rcd == 0 and np.array_equal(back, sym), c.name
        _check_aim(c, u, blob)


def test_the_tables_are_permutations_with_the_reference_invariants():
    """buildCTable / buildDtable of the model on one case per table shape: every state once, every symbol's states ascending"""
    for name in ("one-bitmap-word/2", "slots-1-2-16-17-64-65/2/tl8", "481x17-slots/2/tl13"):
        u = S.unit(next(c for c in CASES if c.name == name))
        size = 1 << u.tl
        state_tab, tt_nb, tt_find, _ = M.ctable(u.norm, u.tl)
        assert sorted(state_tab.tolist()) == list(range(size, 2 * size))
        tab_sym, dt = M.dtable(u.norm, u.tl)
        assert np.array_equal(np.bincount(tab_sym, minlength=u.symbol_len), M._slots(u.norm))
        assert ((dt & 0xFFFF) < size).all() and ((dt >> 16) <= u.tl).all()
        rs, rd = M.rans_dtable(u.norm, u.tl)
        assert rs.size == size and np.array_equal(np.bincount(rs, minlength=u.symbol_len), M._slots(u.norm))
