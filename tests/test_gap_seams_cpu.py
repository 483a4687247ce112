"""What tests/test_gpu_gap_seams.py rests on, checked without a device (tests/gap_seam_frames.py): every frame HAS the property it is
named for -- read from the oracle's tokens of the frame by the model of k_enc_gap's walk, not from how the frame was built -- every
frame codes in the restatement (tests/gap_ref.py) with the status, mode byte, header length, blob length and blob hash on record in
tests/golden/gap_seam_cases.json for 2, 4 and 8 states, the reference's decoder takes every blob back to the frame, and the set as a
whole reaches every seam of SEAMS.  No case is skipped; every case is meant to code, so every status is 0.

One seam of the list the kernel cannot have: an escape whose predecessor is another thread of the SAME wave.  A wave holds 256 bins, so
the widest gap inside one is 254 (bins 0 and 255) and an escape needs 255; the model proves it for every case and the set holds the
254 instead (escape/widest_gap_inside_a_wave).

The model's own words are held to the restatement too: the delta map assembled from the positions the model gives, entry by entry,
is gap_ref.delta_map's, and the histogram compacted in place by the kernel's zeroing rule is the compact histogram with nothing left
behind it -- while the same rule moved by one bin at its upper end leaves a dirty bin or loses a count in at least one case, which is
what lets the device tests see such a slip."""
import re

import numpy as np
import pytest

import gap_ref
import gap_seam_frames as G

NAMES = G.names()


def _esc_of(m, v):
    return next((x for x in m["escapes"] if x.value == v), None)


@pytest.mark.parametrize("name", NAMES)
def test_a_case_has_the_property_it_is_named_for(mico, name):
    _check_claims(G.case(name), G.case(name).facts(mico))


def _check_claims(c, f):
    e, m, cl = f["e"], f["model"], c.claims
    pred = {v: p for p, v in zip(e, e[1:])}
    assert e[-1] == G.delim_of(c.maxv) and e[-1] < f["hi"] and m["steps"] == f["hi"] // G.GAP_CHUNK
    assert not any(x.where == "wave" for x in m["escapes"])               # (no escape has its predecessor in its own wave)
    assert cl, "a case without a claim"
    for kind, vs in cl.get("pairs", {}).items():
        for v in vs:
            assert v in e and v + 1 in e, (kind, v)
            at_step, at_wave = v % G.GAP_CHUNK == G.GAP_CHUNK - 1, v % G.WAVE_BINS == G.WAVE_BINS - 1
            assert {"step": at_step, "wave": at_wave and not at_step, "thread": v % 4 == 3 and not at_wave}[kind], (kind, v)
    for v, g in cl.get("gaps", {}).items():
        assert v in pred and v - pred[v] - 1 == g and (_esc_of(m, v) is not None) == (g >= 255), (v, g)
    for v in cl.get("same_wave", ()):
        assert v // G.WAVE_BINS == pred[v] // G.WAVE_BINS and _esc_of(m, v) is None and v - pred[v] - 1 == 254
    for v, (where, idle) in cl.get("where", {}).items():
        x = _esc_of(m, v)
        assert x is not None and (x.where, x.idle) == (where, idle), (v, x)
    for s, vs in cl.get("in_step", {}).items():
        xs = [x for x in m["escapes"] if x.step == s]
        assert [x.value for x in xs if x.value in vs] == vs and len({_esc_of(m, v).wave for v in vs}) == len(vs), (s, xs)
        for a, b in zip(vs, vs[1:]):
            assert any(a < v < b and _esc_of(m, v) is None for v in e), (a, b)
    for v, before in cl.get("first_of_step", {}).items():
        x = _esc_of(m, v)
        assert x is not None and x.first_of_step and x.before == before >= 1, (v, x)
    assert f["mode"] == cl["mode"] and f["apply"] == (cl["mode"] != 0)
    if "chosen" in cl:
        assert f["chosen"] == cl["chosen"]
    if "decision" in cl:                                                  # (slack, used, escapes, the smallest map)
        assert (f["slack"], len(e), len(m["escapes"]), f["chosen"]) == cl["decision"] and f["half"] and f["delta"] == f["best"]
        assert f["slack"] == 4064 - 9 * len(e) - 16 * len(m["escapes"])
    if "raw_minus_delta" in cl:
        assert f["raw"] - f["delta"] == cl["raw_minus_delta"] and f["bitmap"] > f["raw"]
    if cl.get("chosen") == gap_ref.MODE_BITMAP:
        assert f["bitmap"] < min(f["raw"], f["delta"]) and f["half"] and len(e) > 1
    if "dense" in cl:                                                     # (first, last of the run of consecutive bins, used values in all)
        lo, hi, used = cl["dense"]
        assert e[:hi - lo + 1] == list(range(lo, hi + 1)) and hi + 1 not in e and len(e) == used <= hi - lo + 1 + 20
        assert sum(1 for v in e if v >= G.GAP_CHUNK) >= 4 or m["busy"] == [0]
    if "used_is_used" in cl:
        assert len(e) == cl["used_is_used"] and len(e) in e and len(e) - 1 in e and m["busy"] == [0] and len(e) % 4 == 0
    if "max_value_token" in cl:
        assert c.maxv == cl["max_value_token"] and c.maxv in e and c.maxv & (c.maxv + 1)
    if "only_delimiter_in_step" in cl:
        s = cl["only_delimiter_in_step"]
        assert m["steps"] == s + 1 and m["per_wave"][s] == [0, 0, 0, 1] and e[-1] // G.GAP_CHUNK == s
    if "last_bin_of_tier1" in cl:
        assert e[-1] == G.TIER1_SYMS - 1 == f["hi"] - 1


def test_every_case_codes_as_recorded_and_the_reference_decodes_it(mico):
    rec = G.golden()
    assert set(rec) == {f"{n}/{ns}" for n in NAMES for ns in G.NSTATES}
    modes = set()
    for c in G.cases():
        for ns in G.NSTATES:
            got = G.record_of(mico, c, ns)
            assert got == rec[f"{c.name}/{ns}"], (c.name, ns, got)
            assert got["status"] == 0 and got["mode"] == c.claims["mode"], (c.name, ns)
            modes.add(got["mode"])
        rc, blob, info = G.reference(mico, c, 2)
        assert blob[0] == c.claims["mode"] and info["header_len"] == (f_best(c, mico) if blob[0] else 1)
        rc, px = gap_ref.decompress(mico, blob, c.w, c.h)
        assert rc == 0 and np.array_equal(px, c.px), c.name
    assert modes == {0x00, 0x01, 0x03}


def f_best(c, mico):
    return c.facts(mico)["best"]


def test_the_set_reaches_every_seam(mico):
    hit = {}
    for c in G.cases():
        for s in G.seams_of(c, c.facts(mico)):
            hit.setdefault(s, []).append(c.name)
    for s in G.SEAMS:
        print(s, "<-", ", ".join(hit.get(s, [])))
    assert sorted(set(G.SEAMS) - set(hit)) == [] and set(hit) <= set(G.SEAMS)
    assert {G.depth_of(c.maxv) for c in G.cases()} >= {12, 13, 14, 16}
    # the escape and the decision cases, at least, go through 2, 4 and 8 states: the record holds all three for every case
    assert all(f"{c.name}/{ns}" in G.golden() for c in G.cases() for ns in G.NSTATES)


def test_the_models_delta_map_is_the_restatements(mico):
    """entry i at 5 + (i - 1) + 2 * (escapes before it), the mode byte counted"""
    seen = 0
    for c in G.cases():
        f = c.facts(mico)
        assert G.model_delta_map(f["e"], f["hi"]) == b"\x03" + gap_ref.delta_map(f["e"]), c.name
        seen += f["apply"] and f["mode"] == gap_ref.MODE_DELTA and any(x.before >= 3 for x in f["model"]["escapes"])
    assert seen >= 5


def test_the_zeroing_rule_leaves_the_compact_histogram_and_a_rule_one_bin_off_does_not(mico):
    dirty, lost = [], []
    for c in G.cases():
        f = c.facts(mico)
        if not f["apply"]:
            continue
        hist = np.bincount(f["tokens"], minlength=f["hi"])
        want = np.zeros(f["hi"], np.int64)
        want[:len(f["e"])] = hist[f["e"]]
        assert np.array_equal(G.model_compaction(hist, f["hi"]), want), c.name
        wide, narrow = G.model_compaction(hist, f["hi"], hi_shift=1), G.model_compaction(hist, f["hi"], hi_shift=-1)
        if wide[(len(f["e"]) + 3) // 4 * 4:].any():                          # (k_enc_hist_clean clears whole vectors of four bins)
            dirty.append(c.name)                                          # a bin behind them keeps a count: the next frame of the slot sees it
        if (narrow[:len(f["e"])] != want[:len(f["e"])]).any():
            lost.append(c.name)                                           # a count zeroed by one thread while another writes it
    print("a rule one bin wider leaves a dirty bin in:", dirty, "-- one bin narrower races for a count in:", lost)
    assert "dense/one_step_depth10" in dirty and {"dense/one_step_depth10", "dense/prefix_from_3"} <= set(lost)


def test_the_wide_alphabet_stream_needs_the_large_tables_and_the_reference_decodes_it(mico):
    px, stream, e, table_log = G.wide_alphabet(mico)
    assert px.shape == (1, 153601) and len(e) > G.TIER1_SYMS and stream[0] == gap_ref.MODE_RAW and table_log >= 14
    assert not gap_ref.choose(mico.delta_rle_compress(px, 65535))[0]      # (the encoder itself does not apply a map here)
    rc, back = gap_ref.decompress(mico, stream, px.shape[1], 1)
    assert rc == 0 and np.array_equal(back, px)


def test_the_crafted_maps_decode_in_the_reference_as_their_names_say(mico):
    sh, dp, maps = G.crafted_maps(mico)
    corrupt = {"delta/0_to_65534", "delta/num_symbols_1", "delta/deep_num_symbols_1"}
    for name, (stream, which, want) in maps.items():
        px = sh if which == "shallow" else dp
        rc, back = gap_ref.decompress(mico, stream, px.shape[1], px.shape[0])
        assert rc == want == (gap_ref.ERR_CORRUPT if name in corrupt else 0), (name, rc)
        assert rc != 0 or np.array_equal(back, px), name
    assert {n.split("/")[0] for n in maps} == {"bitmap", "raw", "delta"}
    hdr = {n: gap_ref.parse_map(s)[1] for n, (s, _, _) in maps.items()}
    assert {hdr[n] - 3 for n in maps if n.startswith("bitmap/bytes_")} == {2, 32, 63, 64, 65, 127, 128, 129, 8192}
    assert {int(n.rsplit("_", 1)[1]) % 8 for n in maps if n.startswith("bitmap/max_sym_")} == set(range(8))
    for n in maps:
        if n.startswith("bitmap/max_sym_"):                               # bits behind maxSym are set, and are no symbols
            s, r = maps[n][0], int(n.rsplit("_", 1)[1]) % 8
            assert r == 7 or s[hdr[n] - 1] >> (r + 1) == 0xFF >> (r + 1)
    for k in (8191, 8192, 8193, 65535):
        assert len(gap_ref.parse_map(maps[f"raw/entries_{k}"][0])[0]) == len(gap_ref.parse_map(maps[f"raw/deep_entries_{k}"][0])[0]) == k
    assert gap_ref.parse_map(maps["bitmap/full"][0])[0] == list(range(65536)) == gap_ref.parse_map(maps["delta/0_to_65534"][0])[0] + [65535]
    assert len(gap_ref.parse_map(maps["delta/long_tail"][0])[0]) > 2 * G.TIER1_SYMS
    assert hdr["delta/all_escaped"] - hdr["delta/none_escaped"] == 2 * (len(gap_ref.parse_map(maps["delta/none_escaped"][0])[0]) - 1)
    assert hdr["delta/none_escaped"] < hdr["delta/some_escaped"] < hdr["delta/all_escaped"]
    assert all(len(gap_ref.parse_map(maps[n][0])[0]) == 1 for n in ("delta/num_symbols_1", "delta/deep_num_symbols_1"))


def test_the_truncation_sweeps_cover_every_prefix_and_both_checks_of_the_delta_walk(mico):
    px, sweeps = G.truncations(mico)
    assert set(sweeps) == {"raw", "bitmap", "delta", "delta_escaped"}
    for form, (stream, hdr) in sweeps.items():
        st = [gap_ref.decompress(mico, stream[:n], px.shape[1], px.shape[0])[0] for n in range(hdr + 2)]
        assert all(s != 0 for s in st) and gap_ref.decompress(mico, stream, px.shape[1], px.shape[0])[0] == 0, form
        assert all(gap_ref.parse_map(stream[:n]) is None for n in range(hdr)) and gap_ref.parse_map(stream[:hdr])[1] == hdr, form


def test_the_models_constants_are_the_sources(mic):
    """the constants the model restates, read back from the sources they name"""
    import os
    src = os.path.join(os.path.dirname(os.path.abspath(mic.__file__)), "csrc")
    text = {n: open(os.path.join(src, n)).read() for n in ("mic_gap.hip", "mic_session.h", "mic_encode.hip", "mic_api.hip")}

    def define(name, where):
        return re.search(r"#define\s+%s\s+(.+?)\s*(//.*)?$" % name, text[where], re.M).group(1)
    assert int(define("GAP_THREADS", "mic_gap.hip")) == G.GAP_THREADS and define("GAP_CHUNK", "mic_gap.hip") == "(GAP_THREADS * 4)"
    assert define("GAP_WAVES", "mic_gap.hip") == "(GAP_THREADS / 64)" and G.GAP_CHUNK == 4 * G.GAP_THREADS
    assert "(uint32_t)(first - prev - 1) >= 255u" in text["mic_gap.hip"] and "at = 5u + (idx - 1u) + 2u * esc0" in text["mic_gap.hip"]
    assert "if (v < c_used || v >= c_used + used_all) hist[v] = 0u;" in text["mic_gap.hip"]
    assert "best * 8u < sym_len - used" in text["mic_gap.hip"] and "if (delta < best)" in text["mic_gap.hip"]
    assert "return tier == 1 ? 8192 : 65536;" in text["mic_session.h"] and int(define("TK_HWIN", "mic_encode.hip")) == G.TIER1_SYMS
    assert "deep |= units[i].max_value >= (1u << 13);" in text["mic_api.hip"]
    assert [G.hist_hi(v) for v in (1023, 4095, 8191, 8192, 9999, 16383, 65535)] == [8192, 8192, 8192, 16384, 16384, 16384, 65536]
    assert [G.tier_of(v) for v in (4095, 8191, 8192, 65535)] == [1, 1, 2, 2]
