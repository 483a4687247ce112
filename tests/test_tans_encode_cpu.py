"""The cases of tests/tans_encode_streams.py and the model of tests/tans_encode_model.py, held against the oracle with no device.

For every case: (a) the oracle alone (mico.fse_compress_tl, asked flavour by flavour for the chain cases) ends as the case is named
to end; (b) the model's blob equals the oracle's byte for byte, so the model that predicts MicUnit.enc_kernel and enc_rounds for
tests/test_gpu_tans_encode.py is checked against the reference and never against the code under test; (c) the case reaches the seam
its `aim` names, worked out again from the model's walk: nblk, per, lastown, n mod BLK, the class, the rounds, the zero-bit threads,
the single-word bitstream.

What the families could not reach, stated here so that nobody lowers a condition silently:
  * the 1024-thread instance codes tableLog 16 only, which takes more than 2^18 tokens (tableLog <= highbit(n - 1) - 2): its
    smallest `per` is 9, so nblk of T - 1, T and T + 1 do not exist for it; the group takes 9 T - 1, 9 T, 9 T + 1 and per 12 instead;
  * a unit of the 512-thread instances with one block of 32 tokens cannot succeed (an alphabet past 1024 symbols costs a header of
    2 n bytes by itself): that case runs the walk and ends in the size verdict;
  * 2 -> 1 by a LENGTH gate needs n = 1, which the table stage refuses: 2 -> 1 is reached by the size verdict instead."""
import numpy as np
import pytest

import tans_encode_model as E
import tans_encode_streams as S

CASES = S.cases()
IDS = [c.name for c in CASES]


def _inner_zero(w):
    """threads that own tokens, hold no bit and lie between threads that hold bits"""
    return [t for t in sorted(w.zero_threads) if (w.mybits[:t] > 0).any() and (w.mybits[t + 1:w.lastown] > 0).any()]


def _lead(u):
    """te_encode's `lead`: bytes from the 16-byte boundary in front of the bitstream, which lies 6 + hdr_len bytes into a staging blob"""
    assert E.STAGING_ALIGN % 16 == 0
    return (6 + u.hdr_len) % E.STAGING_ALIGN & 15


def test_the_models_kernel_numbers_are_the_class_bits_of_the_launcher():
    """MicUnit.enc_kernel is 1 + the bit index of MIC_ENC_CLS_* (the kernel derives it from the macros); the model's names follow them"""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "medical-image-codec_amd", "csrc")
    bits = {m[0]: int(m[1], 16) for m in re.findall(r"#define MIC_ENC_CLS_(\w+)\s+0x([0-9a-fA-F]+)u", open(os.path.join(csrc, "mic_launch.h")).read())}
    assert {k: 1 + v.bit_length() - 1 for k, v in bits.items()} == {"NARROW2": E.NARROW2, "WIDE": E.WIDE, "SMALL12": E.SMALL12, "SMALL13": E.SMALL13,
                                                                   "TL14": E.TL14, "TL15": E.TL15, "TL16": E.TL16}, bits
    assert all(v & (v - 1) == 0 for v in bits.values())
    serial = re.search(r"#define MIC_ENC_BY_SERIAL\s+(\d+)u", open(os.path.join(csrc, "mic_dev.h")).read())
    assert int(serial[1]) == E.SERIAL


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_oracle_carries_the_case_and_the_model_writes_its_bytes(mico, case):
    rc, lanes, blob = S.reference(mico, case)
    want = S.ENDS.get(case.name, (0, 8 if case.flavour == 108 else case.flavour))
    assert (rc, lanes) == want, (case.name, "the oracle ends on", rc, lanes, "named", want)          # (a)
    u, r = S.unit(case), S.model(case)
    if u.rc:                                                               # refused in front of the tANS stage: nothing to model
        assert rc == u.rc and r is None, (case.name, rc, u.rc)
        return
    assert (r.status, r.flavour) == (rc, lanes), (case.name, "model", r.status, r.flavour, "oracle", rc, lanes, r.attempts)
    if rc == 0 and r.blob != blob:                                         # (b)
        k = next((k for k in range(min(len(blob), len(r.blob))) if blob[k] != r.blob[k]), min(len(blob), len(r.blob)))
        raise AssertionError((case.name, "first differing byte", k, len(r.blob), len(blob)))
    assert r.kernel != E.SERIAL and 1 <= r.rounds <= r.walk.T


@pytest.mark.parametrize("case", [c for c in CASES if c.group == "partition"], ids=[c.name for c in CASES if c.group == "partition"])
def test_partition_cases_reach_their_block_counts(mico, case):
    _, T, BLK, nblk, per = case.aim
    w = S.model(case).walk
    assert (w.T, w.BLK, w.nblk, w.per) == (T, BLK, nblk, per), (case.name, w.T, w.BLK, w.nblk, w.per)
    assert w.nblk == -(-S.unit(case).n // BLK) and w.per == -(-nblk // T) and w.lastown == -(-nblk // per)


def test_the_partition_group_covers_every_length_that_matters():
    for T, BLK, _ in S.PARTITION:
        ws = [(S.unit(c).n, S.model(c).walk) for c in S.group("partition") if c.aim[1:3] == (T, BLK)]
        rgrp, warm = 128 // BLK, 128 // BLK
        nblks = {w.nblk for _, w in ws}
        want = {9 * T - 1, 9 * T, 9 * T + 1} if T == 1024 else {1, T - 1, T, T + 1, 2 * T, 2 * T + 1}
        assert want <= nblks, (T, BLK, sorted(want - nblks))
        assert {0, 1, BLK - 1} <= {n % BLK for n, _ in ws}, (T, BLK, "n mod BLK")
        pers = {w.per for _, w in ws}
        assert any(p % rgrp for p in pers) and any(p % rgrp == 0 for p in pers), (T, BLK, "whole and partial record groups", pers)
        if T != 1024:
            assert {rgrp, rgrp + 1} <= pers, (T, BLK, pers)
            assert any(w.per < warm for _, w in ws), (T, BLK, "a warm-up that reaches past the predecessor's whole range")
        assert any(w.lastown < T for _, w in ws), (T, BLK, "idle threads behind the last owner")
        assert any(w.nblk - (w.lastown - 1) * w.per < w.per for _, w in ws), (T, BLK, "a last owner with fewer than per blocks")
        # the warm-up of thread 1 is clipped by the end of the stream (w_hi = min(b_hi + WARM, nblk)) whenever per < WARM, and walks
        # the bounded last block whenever n mod BLK != 0
        assert any(w.per < warm and n % BLK for n, w in ws) or T == 1024
        assert any((w.nblk - w.per) + warm > w.nblk for _, w in ws) or T == 1024


@pytest.mark.parametrize("case", [c for c in CASES if c.group == "classes"], ids=[c.name for c in CASES if c.group == "classes"])
def test_class_cases_sit_on_their_side_of_the_border(mico, case):
    _, what, value, k2, k = case.aim
    u, r = S.unit(case), S.model(case)
    assert {"ntok": u.n, "symbol_len": u.symbol_len, "table_log": u.tl}[what] == value, (case.name, u.n, u.symbol_len, u.tl)
    assert r.kernel == (k2 if case.flavour == 2 else k), (case.name, E.KERNELS[r.kernel])
    assert r.status == 0 and not r.handed


def test_the_class_group_has_both_sides_of_every_border_in_every_flavour():
    seen = {}
    for c in S.group("classes"):
        seen.setdefault((c.aim[1], c.aim[2]), set()).add(c.flavour)
    for what, a, b, flavours in (("ntok", 98304, 98305, {1, 2, 4, 8, 108}), ("symbol_len", 512, 513, {1, 2, 4, 8, 108}),
                                 ("symbol_len", 1024, 1025, {1, 2, 4, 8, 108}), ("symbol_len", 4096, 4097, {1, 2, 4, 8, 108}),
                                 ("table_log", 12, 13, {1, 2, 4, 8, 108}), ("table_log", 13, 14, {1, 2, 4, 8, 108}),
                                 ("table_log", 14, 15, {1, 2, 4, 8, 108}), ("table_log", 15, 16, {1, 2, 4, 8, 108})):
        assert flavours <= seen[(what, a)] and flavours <= seen[(what, b)], (what, a, b, seen[(what, a)], seen[(what, b)])
    # ... on either side of tableLog 12 / 13 and 13 / 14 in the one-wave instances AND in the 512-thread ones, 14 / 15 with records in LDS and gathered
    for name, tls in (("small-alphabet", (12, 13)), ("300k", (13, 14, 15, 16)), ("300k-5000-symbols", (14, 15))):
        for tl in tls:
            assert {c.flavour for c in S.group("classes") if c.name.startswith(name + "/") and c.req_tl == tl} == {1, 2, 4, 8, 108}, (name, tl)
    kernels = {S.model(c).kernel for c in S.group("classes")}
    assert kernels == {E.NARROW2, E.WIDE, E.SMALL12, E.SMALL13, E.TL14, E.TL15, E.TL16}
    hbm = [c for c in S.group("classes") if S.unit(c).symbol_len > E.TT_SYMS]          # coding records gathered from HBM
    assert {S.model(c).kernel for c in hbm} >= {E.WIDE, E.TL14, E.TL15}


@pytest.mark.parametrize("case", [c for c in CASES if c.group == "fixup"], ids=[c.name for c in CASES if c.group == "fixup"])
def test_fixup_cases_go_where_they_aim(mico, case):
    u, r = S.unit(case), S.model(case)
    w = r.walk
    assert r.status == 0 and w.T == (case.aim[1] if case.aim[0] != "unit-border" else 64)
    if case.aim[0] == "dominant":
        usual = S.model(S.by_name(case.aim[2]))
        assert usual.kernel == r.kernel and S.unit(S.by_name(case.aim[2])).n == u.n
        assert r.rounds > 2 and r.rounds >= 4 * usual.rounds, (case.name, r.rounds, "image-like", usual.rounds)
        assert u.norm[0] > (1 << u.tl) // 2                                # one symbol with more than half the table
        assert _inner_zero(w), (case.name, "no thread without bits between threads with bits")
    elif case.aim[0] == "zero-threads":
        assert r.rounds > 2 and len(_inner_zero(w)) >= 8, (case.name, r.rounds, len(_inner_zero(w)))
    elif case.aim[0] == "unit-border":
        assert (8 * _lead(u) + w.sym_bits) % 64 == case.aim[1], (case.name, _lead(u), w.sym_bits)


def test_the_fixup_group_has_a_dominant_stream_for_every_thread_count():
    assert {c.aim[1] for c in S.group("fixup") if c.aim[0] == "dominant"} == {64, 512, 1024}
    assert {S.model(c).kernel for c in S.group("fixup") if c.aim[0] in ("dominant", "zero-threads")} >= {E.NARROW2, E.WIDE, E.SMALL12, E.TL16}
    assert {c.aim[1] for c in S.group("fixup") if c.aim[0] == "unit-border"} == {0, 1}


def test_the_pack_group_covers_the_shared_words(mico):
    """where each tiny unit's bitstream lies in the packed buffer (8-byte aligned; a unit starts where its predecessor ends)"""
    off, starts, inside, on_start, on_end, kinds = 0, set(), 0, 0, 0, []
    cs = S.group("pack")
    for c in cs:
        rc, lanes, blob = S.reference(mico, c)
        kinds.append("fails" if rc else "tiny" if c.aim == ("tiny",) else "other")
        if rc:
            continue
        if c.aim == ("tiny",):
            u, r = S.unit(c), S.model(c)
            assert r.kernel == E.NARROW2 and u.symbol_len > 1024 and u.n < 128 and r.walk.total_bytes < 16, (c.name, u.n, r.walk.total_bytes)
            a, b = off + 6 + u.hdr_len, off + len(blob)
            assert b - a == r.walk.total_bytes
            starts.add(a % 8)
            inside += a // 8 == (b - 1) // 8 and a % 8 != 0 and b % 8 != 0
            on_start += a % 8 == 0
            on_end += b % 8 == 0
        off += len(blob)
    assert starts == set(range(8)), sorted(starts)
    assert inside and on_start and on_end, (inside, on_start, on_end)
    assert "fails" in kinds and kinds[0] == kinds[-1] == "tiny"
    others = {S.model(c).kernel for c in cs if c.aim != ("tiny",) and S.model(c) is not None}
    assert others >= {E.SMALL12, E.WIDE, E.TL14}, others
    for i, k in enumerate(kinds):                                           # every other unit and the failing one lie between tiny ones
        if k != "tiny":
            assert kinds[i - 1] == "tiny" and kinds[i + 1] == "tiny", (i, kinds)


@pytest.mark.parametrize("case", [c for c in CASES if c.group == "chain"], ids=[c.name for c in CASES if c.group == "chain"])
def test_chain_cases_fall_where_they_aim(mico, case):
    r = S.model(case)
    n = S.unit(case).n
    if case.aim[0] == "handed":
        assert r.handed and r.kernel == E.WIDE and r.attempts[0] == (E.NARROW2, 2, E.ERR_INCOMPRESSIBLE), (case.name, r.attempts)
        assert r.attempts[1] == (E.WIDE, 2, E.ERR_INCOMPRESSIBLE)          # the wide instance starts over
        assert (r.status == 0 and r.flavour == 1) == case.aim[1], (case.name, r.status, r.flavour)
    elif case.aim[1] == "length gate":
        _, _, a, b = case.aim
        assert n == a - 1 and r.attempts[0][1:] == (a, E.ERR_INCOMPRESSIBLE) and r.attempts[1][1] == b and r.attempts[0][0] == r.attempts[1][0]
        assert not r.handed
    elif case.aim[1] == "size verdict":
        assert [x[1] for x in r.attempts] == [2, 1] and r.attempts[0][2] == E.ERR_INCOMPRESSIBLE and r.walk is not None
    else:
        assert len(r.attempts) == 1 and r.status == 0 and r.flavour == case.flavour
