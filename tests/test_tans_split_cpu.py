"""The CPU model of the split two-state decode (tests/tans_split_model.py) against the oracle's own streams: its plain decode gives
the oracle's tokens, the two halves of the headline's strips meet inside the default overlap, and the gate keeps low-rate streams
(where a wrong start is not forgotten in time) away from the split instance.  No GPU."""
import functools
import json
import os
import zlib

import numpy as np
import pytest

import tans_split_model as M
import test_gpu_tans_split as S2                   # (its unit builders; nothing of it runs here)

RECORDS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tans_split_records.json")


def _strip(synth, seed, strip, rows=256, noise=None):
    noise = synth.XR_NOISE_PUBLISHED_RATIO if noise is None else noise
    img = synth.xr_like(cols=2577, rows=2048, depth=12, seed=seed, noise=noise)
    return np.ascontiguousarray(img[strip * 256:strip * 256 + rows])


def test_plain_decode_equals_the_oracles_tokens(mico, synth):
    tok = mico.delta_rle_compress(_strip(synth, 1, 3, rows=24), 4095)
    s = M.Stream(mico, tok)
    got, left = s.decode()
    assert np.array_equal(got, tok)
    assert left >= 0
    rc, back = mico.fse_decompress_auto(s.blob, tok.size)
    assert rc == 0 and np.array_equal(back, tok)


@pytest.mark.parametrize("seed,strip", [(1, 0), (100004, 3), (250, 7)])
def test_bench_strips_meet_inside_the_default_overlap(mico, synth, seed, strip):
    tok = mico.delta_rle_compress(_strip(synth, seed, strip), 4095)
    s = M.Stream(mico, tok)
    assert s.table_log == 13 and not s.zero_bits
    assert 9.0 <= 8 * s.nbytes / s.count <= 10.5, 8 * s.nbytes / s.count  # the headline's rate: about 9.6 bits per token
    assert s.gate()
    outcome, i_sync, j_sync = s.split()
    assert outcome == M.DONE, (outcome, i_sync, j_sync)
    assert j_sync == M.OVERLAP and j_sync < i_sync <= (s.count // 64) * 64
    # both parts decode about half the stream plus half the overlap
    assert abs(i_sync - (s.count + M.OVERLAP) // 2) < s.count // 20, (i_sync, s.count)
    # and the meeting is no accident of W: a wrong start is forgotten well inside half of it
    pm = s.split_start(M.OVERLAP)
    _, a, b = s.start(pm)
    d = s.meeting_distance(pm - 2 * s.table_log, a, b, M.OVERLAP)
    assert d is not None and d <= M.OVERLAP // 2, d


def test_the_gate_refuses_a_low_noise_strip(mico, synth):
    tok = mico.delta_rle_compress(_strip(synth, 1, 3, noise=3.0), 4095)
    s = M.Stream(mico, tok)
    assert s.count >= M.MIN_TOKENS
    assert 8 * s.nbytes / s.count < 9.0
    assert not s.gate()


def test_a_short_stream_is_not_tried(mico, synth):
    tok = mico.delta_rle_compress(_strip(synth, 1, 3, rows=24), 4095)
    s = M.Stream(mico, tok)
    assert s.count < M.MIN_TOKENS and not s.gate()
    assert s.gate(min_tokens=4096)


def test_an_overlap_too_small_to_meet_in_falls_back(mico, synth):
    tok = mico.delta_rle_compress(_strip(synth, 5, 3, rows=24), 4095)   # (64 symbols can be enough by luck: seed 1's strip meets after 16)
    s = M.Stream(mico, tok)
    assert s.split(W=64) == (M.NOT_MET, 0, 64)
    assert s.split(W=4096)[0] == M.DONE


@functools.lru_cache(maxsize=None)
def _recorded_unit(mico, synth, seed, rows, noise, residue):
    img = S2._strip(synth, seed, rows, noise=noise)
    return S2.Unit(mico, img if residue is None else S2._with_tokens(mico, img, residue))


def test_the_model_reproduces_the_recorded_outcomes(mico, synth):
    """tests/golden/tans_split_records.json holds what the two former models (a two-part and a four-part one, at commit f00724c) made
    of the units of test_gpu_tans_split.py and test_gpu_tans_split4.py -- candidates, tile-edge cases, the strip that does not meet,
    at the overlaps those files use, and a few with a scratch capacity (`cap`: two parts' slab, four parts' R) small enough to run
    out of room; the one model must give every record again."""
    seen = set()
    for e in json.load(open(RECORDS)):
        u = _recorded_unit(mico, synth, e["seed"], e["rows"], e["noise"], e["residue"])
        s, W = u.model, e["overlap"]
        assert s.count == e["tokens"], e
        if e["parts"] == 2:
            got = s.split(W, cap=e["cap"]) if s.gate(min_tokens=S2.MIN_TEST) else (M.NOT_TRIED, 0, 0)
            assert got == (e["outcome"], e["i_sync"], e["j_sync"]), (e, got)
        else:
            R = M.region(u.img.size) if e["cap"] is None else e["cap"]
            got = M.split_parts(s, W, R=R)
            assert R == e["R"] and got == (e["outcome"], tuple(e["I"]), e["fail"]), (e, got)
            if e["crc32"] is not None:
                states, I = M.joined(s, W)
                assert tuple(I) == tuple(e["I"]) and zlib.crc32(np.asarray(states, np.uint16).tobytes()) == e["crc32"], e
        seen.add((e["parts"], e["outcome"]))
    assert seen >= {(n, o) for n in (2, 4) for o in (M.DONE, M.NOT_MET, M.NO_ROOM)}, seen
