"""The gap-removal kernels at their seams (csrc/mic_gap.hip: k_enc_gap, k_enc_gap_remap, k_enc_gap_len, k_dec_gap_map,
k_dec_gap_expand; k_dec_gap_check in csrc/mic_decode.hip), one hand-built input per seam (tests/gap_seam_frames.py; what the inputs
are and that they have the properties they are named for is tests/test_gap_seams_cpu.py's business).  Everything is exact: bytes,
statuses and pixels are those of the restatement in tests/gap_ref.py on top of the oracle.

  Encode: used values on both sides of a step (1024 bins), wave (256) and thread (4) edge of k_enc_gap's walk, at depth 12 and in the
  late steps of depth 16; gaps of 253, 254, 255 and 256 and one whose escape bytes differ; an escape whose predecessor lies in
  another wave of its step, in the step before and many idle steps back; four escapes in one step with plain entries between them
  and steps that begin with an escape when the scan has counted several; a dense prefix with compact index == value, and three behind
  it, while the histogram moves in place; every token in one step with the bins numUsed - 1 and numUsed used themselves; the decision
  on the tie (not applied), one above it (applied), raw == delta (raw), delta one under raw, and the bitmap smallest (never applied);
  depths 10, 12, 13 (the delimiter in the last bin of the small slab), 14 (a max_value that is no 2^k - 1) and 16 (64 steps, the last
  with the delimiter alone), the last two in the large slabs; 2, 4 and 8 states.  Through compress_single_frame_gap_removal and
  a session unit with MIC_HIP_GAP_REMOVAL, all cases of a tier in one batch and in reverse order (the units side by side in the gap
  slab), and frame after frame in one session slot between plain frames of another shape, which is what sees a histogram bin left
  dirty behind the compaction (the session keeps the slabs zero instead of clearing them).
  Decode: bitmaps of 2 .. 8192 bytes (lanes of k_dec_gap_map left empty, every bit in one lane's run), maxSym at every residue with
  the bits behind it set, raw and delta maps longer than the table of the tier (8191, 8192, 8193, 65535 entries; the expand table is
  followed by other units' slabs), the identity maps in front of a plain stream, delta maps with none, some and all entries escaped
  and with one entry, a compact alphabet of 8404 symbols that only the large tables hold, every prefix of one stream of each form,
  and the weighted-but-unemitted stream of k_dec_gap_check among them; alone, in one batch between ordinary gap streams, and in a
  session whose output tensor ends in 4096 samples of 0xA5A5.

Two branches of k_enc_gap no door reaches, and nothing here tries to: `hi` not a multiple of four (hi is 8192 or a larger power of
two) and a WRITTEN bitmap map (a chosen bitmap never passes the test that applies a map)."""
import numpy as np
import pytest

import gap_ref
import gap_seam_frames as G
from test_gap_removal_ref import near_constant
from test_gpu_gap_removal import _weighted_unused

pytestmark = pytest.mark.gpu

CANARY = 4096
FILL = 0xA5A5


def _want(mico, c, ns):
    """the restatement's (status, blob), held to the record"""
    rc, blob, _ = G.reference(mico, c, ns)
    g = G.golden()[f"{c.name}/{ns}"]
    assert (rc, len(blob), f"{mico.fnv1a64(blob):016x}") == (g["status"], g["blob_len"], g["blob_fnv1a64"]), (c.name, ns)
    return rc, blob


def _single(mic, px, maxv, ns):
    try:
        return 0, mic.compress_single_frame_gap_removal(px, px.shape[1], px.shape[0], maxv, ns)
    except mic.MicError as e:
        return e.code, b""


def _decode(mic, blob, w, h):
    try:
        return 0, mic.decompress_single_frame_gap_removal(blob, w, h)
    except mic.MicError as e:
        return e.code, None


def _session_encode(mic, torch, sess, frames, maxvs, nstates):
    """-> (status per unit, blob per unit, the device blobs, their offsets, the units): nstates carries the units' flags"""
    flat = np.concatenate([np.ascontiguousarray(f, dtype=np.uint16).reshape(-1) for f in frames])
    d_px = torch.from_numpy(flat.view(np.int16)).cuda()
    starts = np.concatenate([[0], np.cumsum([f.size for f in frames])])
    units = mic.Session.make_units([(int(starts[i]), f.shape[1], f.shape[0], maxvs[i], nstates[i]) for i, f in enumerate(frames)])
    sess.encode_enqueue(d_px.data_ptr(), units)
    d, offs, st, _ = sess.encode_finish()
    total = int(offs[-1])
    dev = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
    if total:
        mic.device_copy(dev.data_ptr(), d, total)
    host = dev.cpu().numpy()
    return [int(s) for s in st], [host[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(frames))], dev, offs, units


def _session_decode(mic, torch, sess, blobs, dims, flags):
    """-> (status per unit, pixels per unit, the tail behind the last unit's pixels)"""
    lens = [len(b) for b in blobs]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    host = np.zeros(int(offs[-1]) + 64, np.uint8)
    host[:int(offs[-1])] = np.frombuffer(b"".join(blobs), np.uint8)
    d_blob = torch.from_numpy(host).cuda()
    starts = np.concatenate([[0], np.cumsum([w * h for w, h in dims])])
    d_out = torch.full((int(starts[-1]) + CANARY,), FILL - 65536, dtype=torch.int16, device="cuda")
    units = mic.Session.make_units([(int(starts[i]), w, h, 0, 2 | flags[i]) for i, (w, h) in enumerate(dims)])
    sess.decode_enqueue(d_blob.data_ptr(), offs, units, d_out.data_ptr())
    st = sess.decode_finish()
    out = d_out.cpu().numpy().view(np.uint16)
    return [int(s) for s in st], [out[int(starts[i]):int(starts[i + 1])].reshape(h, w) for i, (w, h) in enumerate(dims)], out[int(starts[-1]):]


@pytest.mark.parametrize("name", G.names())
def test_a_seam_case_codes_to_the_restatements_bytes_through_both_doors(gpu_ready, mic, mico, name):
    torch = pytest.importorskip("torch")
    c = G.case(name)
    want = [_want(mico, c, ns) for ns in G.NSTATES]
    for ns, (rc, blob) in zip(G.NSTATES, want):
        rc_g, got = _single(mic, c.px, c.maxv, ns)
        print(name, ns, "status", rc_g, "bytes", len(got), "reference", rc, len(blob), "mode", blob[:1].hex())
        assert rc_g == rc, (ns, rc_g, rc)
        assert got == blob, (ns, len(got), len(blob), got[:8].hex(), blob[:8].hex())
        if rc == 0:
            rc_d, px = _decode(mic, got, c.w, c.h)
            assert rc_d == 0 and np.array_equal(px, c.px), (ns, rc_d)
    # the same through session units, one per flavour, twice: the session's launch masks all ones, then the learned ones
    flag = mic.MIC_HIP_GAP_REMOVAL
    sess = mic.Session(3, c.w * c.h)
    try:
        for again in range(2):
            st, blobs, dev, offs, units = _session_encode(mic, torch, sess, [c.px] * 3, [c.maxv] * 3, [ns | flag for ns in G.NSTATES])
            assert st == [rc for rc, _ in want], (again, st)
            assert blobs == [blob for _, blob in want], (again, [len(b) for b in blobs])
            st, pxs, tail = _session_decode(mic, torch, sess, blobs, [(c.w, c.h)] * 3, [flag] * 3)
            assert st == [0, 0, 0], (again, st)
            assert all(np.array_equal(p, c.px) for p in pxs) and (tail == FILL).all(), again
    finally:
        sess.close()


@pytest.mark.parametrize("tier", [1, 2])
def test_all_cases_of_a_tier_in_one_batch_and_in_reverse_order(gpu_ready, mic, mico, tier):
    """the units lie side by side in the gap slab (compact-index table, then the map): each blob is the single frame's"""
    cs = [c for c in G.cases() if G.tier_of(c.maxv) == tier]
    assert len(cs) >= 4
    for ns in G.NSTATES:
        want = [_want(mico, c, ns) for c in cs]
        for order in (list(range(len(cs))), list(range(len(cs)))[::-1]):
            res = mic.compress_batch_gap_removal([cs[i].px for i in order], [cs[i].maxv for i in order], ns)
            for i, (st, blob, _) in zip(order, res):
                assert st == want[i][0] and blob == want[i][1], (ns, cs[i].name, st, len(blob), len(want[i][1]))
            dec = mic.decompress_batch_gap_removal([b for _, b, _ in res], [(cs[i].w, cs[i].h) for i in order])
            for i, (st, px) in zip(order, dec):
                assert st == 0 and np.array_equal(px, cs[i].px), (ns, cs[i].name, st)


STALE = {
    1: ("dense/one_step_depth10", "dense/prefix_from_3", "dense/prefix_from_0", "escape/four_in_one_step", "decision/slack_1_is_applied",
        "decision/tie_is_not_applied", "escape/widest_gap_inside_a_wave", "edges/depth12"),
    2: ("escape/carried_depth14", "edges/depth16_late_steps", "depth/14_not_a_power_of_two", "escape/predecessor_far_depth16"),
}


@pytest.mark.parametrize("tier", [1, 2])
def test_a_session_slot_is_clean_behind_every_applied_map(gpu_ready, mic, mico, synth, tier):
    """one session, one unit, frame after frame: a gap frame, then a plain frame of another shape whose tables take in every bin of
    the slab, and so on; the last gap frame's used values lie above the numUsed of the applied map before it.  k_enc_hist_clean
    clears [0, numUsed) behind an applied map, so a bin that the compaction left dirty behind numUsed shows in the next blob."""
    torch = pytest.importorskip("torch")
    depth = 12 if tier == 1 else 16
    cols, rows = (193, 61) if tier == 1 else (257, 190)                   # (large enough to entropy-code at their depth)
    plain = [synth.xr_like(cols=cols + 8 * k, rows=rows + k, depth=depth, seed=20 + k) for k in range(len(STALE[tier]))]
    cs = [G.case(n) for n in STALE[tier]]
    assert all(G.tier_of(c.maxv) == tier for c in cs) and sum(c.facts(mico)["apply"] for c in cs) >= len(cs) - 1
    before = [c for c in cs[:-1] if c.facts(mico)["apply"]][-1]
    assert min(cs[-1].facts(mico)["e"]) > len(before.facts(mico)["e"]) and cs[-1].facts(mico)["apply"]
    sess = mic.Session(1, max([c.w * c.h for c in cs] + [p.size for p in plain]))
    try:
        for k, c in enumerate(cs):
            rc, blob = _want(mico, c, 2)
            st, blobs, _, _, _ = _session_encode(mic, torch, sess, [c.px], [c.maxv], [2 | mic.MIC_HIP_GAP_REMOVAL])
            assert st == [rc] and blobs[0] == blob, (k, c.name, st, len(blobs[0]), len(blob))
            if k + 1 < len(cs):
                p, mv = plain[k], (1 << depth) - 1
                rc, blob = mico.compress_single_frame(p, mv)
                st, blobs, _, _, _ = _session_encode(mic, torch, sess, [p], [mv], [2])
                assert st == [rc] == [0] and blobs[0] == blob, (k, "the plain frame behind " + c.name, st, len(blobs[0]), len(blob))
    finally:
        sess.close()


def _neighbour(mico):
    c = G.case("escape/thresholds")
    return G.reference(mico, c, 2)[1], c


DEEP_PLAIN = ("bitmap/deep_full", "delta/0_to_65534")     # the two whose PLAIN stream has 65536 symbols: the chain runs again in tier 2


def _crafted_jobs(mico, deep_plain, nstates=2):
    """the crafted maps, an ordinary gap stream in front of each and six behind the last (the expand table of a tier-1 unit is 16 KiB
    of its 24 KiB slab: 65535 entries written unclipped would reach into the sixth slab behind), and the weighted-but-unemitted
    stream of k_dec_gap_check.  The two streams that send the whole batch to tier 2 -- where no map is clipped and every unit is
    decoded again -- go in a batch of their own (deep_plain), so the others are judged by their tier-1 run.
    -> [(name, stream, (w, h), reference status, reference pixels)]"""
    sh, dp, maps = G.crafted_maps(mico)
    nb, nc = _neighbour(mico)
    jobs = []
    for name, (stream, which, rc) in maps.items():
        if (name in DEEP_PLAIN) != deep_plain:
            continue
        px = sh if which == "shallow" else dp
        jobs.append(("neighbour", nb, (nc.w, nc.h), 0, nc.px))
        jobs.append((name, stream, (px.shape[1], px.shape[0]), rc, px if rc == 0 else None))
    nconst = near_constant()
    weighted, _, _ = _weighted_unused(mico, nconst, 65535, nstates)
    jobs.append(("weighted_but_unemitted", weighted, (nconst.shape[1], nconst.shape[0]), 0, nconst))
    jobs += [("neighbour", nb, (nc.w, nc.h), 0, nc.px)] * 6
    return jobs


def test_a_crafted_map_decodes_as_the_reference_says(gpu_ready, mic, mico):
    sh, dp, maps = G.crafted_maps(mico)
    assert set(DEEP_PLAIN) <= set(maps)
    for name, (stream, which, rc) in maps.items():
        px = sh if which == "shallow" else dp
        rc_g, got = _decode(mic, stream, px.shape[1], px.shape[0])
        print(name, "status", rc_g, "reference", rc)
        assert rc_g == rc, (name, rc_g, rc)
        assert rc != 0 or np.array_equal(got, px), name


@pytest.mark.parametrize("deep_plain", [False, True])
def test_the_crafted_maps_decode_in_one_batch_between_ordinary_streams(gpu_ready, mic, mico, deep_plain):
    jobs = _crafted_jobs(mico, deep_plain)
    assert len(jobs) < 200
    res = mic.decompress_batch_gap_removal([j[1] for j in jobs], [j[2] for j in jobs])
    for k, ((name, _, _, rc, px), (st, got)) in enumerate(zip(jobs, res)):
        assert st == rc, (k, name, st, rc)
        assert rc != 0 or np.array_equal(got, px), (k, name, "behind " + jobs[k - 1][0] if k else "")


@pytest.mark.parametrize("deep_plain", [False, True])
def test_the_crafted_maps_decode_in_a_session_and_leave_the_tail_alone(gpu_ready, mic, mico, deep_plain):
    """a fresh session starts in tier 1: the long maps are clipped at 8192 entries, the neighbours' slabs behind them stay theirs"""
    torch = pytest.importorskip("torch")
    jobs = _crafted_jobs(mico, deep_plain)
    sess = mic.Session(len(jobs), max(w * h for _, _, (w, h), _, _ in jobs))
    try:
        for again in range(2):
            st, pxs, tail = _session_decode(mic, torch, sess, [j[1] for j in jobs], [j[2] for j in jobs], [mic.MIC_HIP_GAP_REMOVAL] * len(jobs))
            for k, ((name, _, _, rc, px), s, got) in enumerate(zip(jobs, st, pxs)):
                assert s == rc, (again, k, name, s, rc)
                assert rc != 0 or np.array_equal(got, px), (again, k, name, "behind " + jobs[k - 1][0] if k else "")
            assert (tail == FILL).all(), (again, int(np.count_nonzero(tail != FILL)))
    finally:
        sess.close()


def test_a_compact_alphabet_wider_than_the_small_tables_decodes(gpu_ready, mic, mico):
    """8404 compact symbols behind a raw map: k_dec_gap_map runs in tier 1 first (the map clipped at 8192 entries), the table kernel
    asks for the large slabs and the whole chain runs again with all of the map"""
    px, stream, e, _ = G.wide_alphabet(mico)
    nb, nc = _neighbour(mico)
    rc, got = _decode(mic, stream, px.shape[1], 1)
    assert rc == 0 and np.array_equal(got, px)
    res = mic.decompress_batch_gap_removal([nb, stream, nb], [(nc.w, nc.h), (px.shape[1], 1), (nc.w, nc.h)])
    assert [st for st, _ in res] == [0, 0, 0]
    assert np.array_equal(res[0][1], nc.px) and np.array_equal(res[1][1], px) and np.array_equal(res[2][1], nc.px)


def test_every_prefix_of_a_map_fails_as_in_the_reference_and_the_whole_stream_decodes(gpu_ready, mic, mico):
    px, sweeps = G.truncations(mico)
    h, w = px.shape
    for form, (stream, hdr) in sweeps.items():
        cuts = [stream[:n] for n in range(hdr + 2)] + [stream]
        want = [gap_ref.decompress(mico, c, w, h)[0] for c in cuts]
        res = mic.decompress_batch_gap_removal(cuts, [(w, h)] * len(cuts))
        print(form, "header", hdr, "reference", want, "device", [st for st, _ in res])
        assert [st for st, _ in res] == want, form
        assert want[-1] == 0 and np.array_equal(res[-1][1], px), form
