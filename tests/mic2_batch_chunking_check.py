"""Run by tests/test_gpu_mic2_batch_seams.py in a child process with MIC_HIP_WS_BUDGET_MB set small (and MIC_HIP_PIPELINE_PARTS=3), so
that the MIC2 whole-volume batches cut their units into sub-batches of two or three.  From the planner's cuts -- which must equal the
restated rule (mic2_multi_volumes.cuts_of) -- the script asserts that a cut falls (a) inside a temporal volume, (b) right behind a
temporal volume's frame 0, (c) between volumes, and (d) so that one sub-batch holds the tail of a temporal volume, a whole independent
volume and the head of the next temporal one; and that a cut falls inside the 16-bit temporal volume, whose sums wrap: the host
doors' sub-batches are their pipeline's parts, so that is where the encoder uploads a lead frame and the decoder carries the running
sum from one staging half to the other.  All four doors must give the single calls' bytes and pixels and count `slabs` as the planner
does; then the run is repeated with frame 5 of the first temporal volume damaged."""
import importlib, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry
mic = entry.load_package(); synth = importlib.import_module("medical_image_codec_amd.synth")
import mic2_batch_volumes as B

budget = int(os.environ.get("MIC_HIP_WS_BUDGET_MB", "0")) << 20
assert budget, "meant to run with a small workspace budget"
made = B.volumes(synth)
made["xr10"] = (np.ascontiguousarray(made["xr12"][0][:10]), made["xr12"][1])
# ten frames three to a sub-batch leave the tenth to share one with the one-frame independent volume and frame 0 of the narrow one
order = [("xr10", True), ("tiny", False), ("narrow", True), ("wrap16", True), ("xr12", False), ("one", True), ("two", True), ("wrap16", False)]
jobs = [(made[k][0], made[k][1], t) for k, t in order]
vols = [j[0] for j in jobs]
files = []
for vol, maxv, t in jobs:
    code, f = B.single_encode(mic, vol, maxv, t)
    assert code == 0
    files.append(f)
units = B.unit_names(vols)
cuts, nunits = mic.mic2_batch_plan([(v.shape[2], v.shape[1], v.shape[0]) for v in vols])   # (the default ceiling is the environment's)
cuts = cuts.tolist()
assert nunits == len(units) and cuts == B.cuts_of(B.units_px(vols), budget), cuts
sizes = [b - a for a, b in zip(cuts, cuts[1:])]
assert set(sizes) <= {1, 2, 3} and 2 in sizes and 3 in sizes, sizes
temporal_of = [t for _, t in order]
seen = set()
for c in cuts[1:-1]:
    v, f = units[c]
    if units[c - 1][0] != v:
        seen.add("c")
    elif temporal_of[v]:
        seen.add("b" if f == 1 else "a")
        if order[v][0] == "wrap16":
            seen.add("wrap")
for a, b in zip(cuts, cuts[1:]):
    groups = []
    for v, f in units[a:b]:
        if groups and groups[-1][0] == v:
            groups[-1][1].append(f)
        else:
            groups.append((v, [f]))
    for (l, lf), (i, fi), (r, rf) in zip(groups, groups[1:], groups[2:]):
        tail = temporal_of[l] and lf[0] > 0 and lf[-1] == vols[l].shape[0] - 1
        head = temporal_of[r] and rf[0] == 0 and rf[-1] < vols[r].shape[0] - 1
        if tail and head and not temporal_of[i] and len(fi) == vols[i].shape[0]:
            seen.add("d")
assert seen == {"a", "b", "c", "d", "wrap"}, (seen, cuts)
slabs = len(cuts) - 1


def device_volumes():
    flat = np.concatenate([v.reshape(-1) for v in vols])
    off, desc = 0, []
    for vol, maxv, t in jobs:
        desc.append((off, vol.shape[2], vol.shape[1], vol.shape[0], maxv, t))
        off += vol.size
    return torch.from_numpy(flat.view(np.int16)).cuda(), desc


# encode: bytes, through the host door (pageable and pinned buffers) and from device memory
res, stats = mic.compress_multi_frame_batch(vols, [j[1] for j in jobs], [j[2] for j in jobs])
assert [r[2] for r in res] == files and stats == dict(units=len(units), slabs=slabs, volumes_done=len(jobs)), stats
pin_in = [mic.host_alloc(v.size * 2, dtype=np.uint16) for v in vols]
pin_out = [mic.host_alloc(mic.mic2_bound(v.shape[2], v.shape[1], v.shape[0])) for v in vols]
for p, v in zip(pin_in, vols):
    p[:] = v.reshape(-1)
res, stats = mic.compress_multi_frame_batch([p.reshape(v.shape) for p, v in zip(pin_in, vols)], [j[1] for j in jobs], [j[2] for j in jobs], outs=pin_out)
assert [r[2] for r in res] == files and stats["slabs"] == slabs
d_px, desc = device_volumes()
enc, dec = mic.Session(4, 160 * 96), mic.Session(4, 160 * 96)
d_files, offs, heads, st, bad, stats = enc.mic2_encode(d_px.data_ptr(), desc)
assert (st == 0).all() and stats == dict(units=len(units), slabs=slabs, volumes_done=len(jobs)), stats
t = torch.empty(int(offs[-1]), dtype=torch.uint8, device="cuda")
mic.device_copy(t.data_ptr(), d_files, int(offs[-1]))
assert t.cpu().numpy().tobytes() == b"".join(files) and heads == [B.Mic2File(f).head() for f in files]


def decode(batch, want, expect):
    """both decode doors on `batch`: volume i must have status / failed frame expect(i) and, when that is MIC_OK, equal want[i]"""
    outs = [np.full(v.size, 0xA5A5, dtype=np.uint16) for v in vols]
    res, stats = mic.decompress_multi_frame_batch(batch, outs=outs)
    assert stats["units"] == len(units) and stats["slabs"] == slabs, stats
    for i, (st, bad, dims, px) in enumerate(res):
        assert (st, bad) == expect(i), (i, st, bad)
        if st == 0:
            assert np.array_equal(px, want[i]), i
    for i, p in enumerate(pin_in):
        p[:] = 0xA5A5
    res, stats = mic.decompress_multi_frame_batch(batch, outs=pin_in)
    assert all((r[0], r[1]) == expect(i) and (r[0] != 0 or np.array_equal(r[3], want[i])) for i, r in enumerate(res)) and stats["slabs"] == slabs
    blobs = [torch.from_numpy(np.frombuffer(f, dtype=np.uint8).copy()).cuda() for f in batch]
    px_off = np.cumsum([0] + [v.size for v in vols])
    d_out = torch.full((int(px_off[-1]) * 2,), 0xA5, dtype=torch.uint8, device="cuda")
    st, bad, stats = dec.mic2_decode([B.Mic2File(f).head() for f in batch], [b.data_ptr() for b in blobs], [len(f) for f in batch],
                                     d_out.data_ptr(), px_off[:-1], int(px_off[-1]))
    assert stats == dict(units=len(units), slabs=slabs, volumes_done=sum(expect(i)[0] == 0 for i in range(len(batch)))), stats
    got = d_out.cpu().numpy().view("<u2")
    for i in range(len(batch)):
        assert (st[i], bad[i]) == expect(i), (i, st[i], bad[i])
        if st[i] == 0:
            assert np.array_equal(got[px_off[i]: px_off[i + 1]], want[i].reshape(-1)), i


decode(files, vols, lambda i: (0, -1))
# ... and the encoder's own device files, as they lie
d_back = torch.full((d_px.numel() * 2,), 0xA5, dtype=torch.uint8, device="cuda")
st, bad, stats = dec.mic2_decode(heads, [d_files + int(o) for o in offs[:-1]], [int(b - a) for a, b in zip(offs, offs[1:])],
                                 d_back.data_ptr(), [d[0] for d in desc], d_px.numel())
assert (st == 0).all() and stats["slabs"] == slabs
assert torch.equal(d_back.view(torch.int16), d_px)

# frame 5 of the first temporal volume damaged: that volume fails (or decodes as the single call does), its later sub-batches do no
# harm and the volumes of later sub-batches are exact
damaged = B.damage(files[0], 5)
code, dec_px = B.single_decode(mic, damaged)
assert any(units[c][0] == 0 and units[c][1] > 5 for c in cuts[1:-1])                       # (the damaged volume goes on in later sub-batches)
want2 = list(vols) if dec_px is None else [dec_px] + vols[1:]
decode([damaged] + files[1:], want2, lambda i: (code, 5) if i == 0 and code else (0, -1))
enc.close(); dec.close()
for p in pin_in + pin_out:
    mic.host_free(p)
print("mic2 batch seams ok")
