"""Patches of many slides and levels per call (csrc/mic_api_ext.hip: mic_hip_wsi_multi_read_patches,
mic_hip_wsi_readers_read_patches).  The expected value of a patch is decompress_wsi_level of its slide and level, padded with zeros
and cropped in numpy (wsi_patch_slides.expected): existing code, never the new path.  The slides (wsi_multi_slides) have three tile
sizes, so one call mixes tiles of 64 x 64, 32 x 48 and 16 x 16 samples in its sub-batches."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import wsi_patch_slides as S
import wsi_multi_slides as M

pytestmark = pytest.mark.gpu

GARBAGE = bytes(range(256)) * 2


@pytest.fixture(scope="module")
def sets(mic, gpu_ready):
    """fmt -> dict(files = [A, B, C], parsed = [Mic3File], levels = [[level image per level] per slide]); decoded once, never written to"""
    out = {}
    for fmt in S.FORMATS:
        files = [M.device_file(mic, name, fmt) for name in M.NAMES]
        parsed = [S.Mic3File(d) for d in files]
        levels = [[mic.decompress_wsi_level(d, l) for l in range(f.nlev)] for d, f in zip(files, parsed)]
        for name, lv in zip(M.NAMES, levels):
            assert np.array_equal(lv[0], M.image(name, fmt)), (fmt, name)
            for a in lv:
                a.setflags(write=False)
        out[fmt] = dict(files=files, parsed=parsed, levels=levels)
    return out


def _bpp(fmt):
    return 3 if fmt == "rgb" else 2 if fmt == "grey16" else 1


def _tensor(n, ph, pw, bpp):
    import torch
    return torch.full((max(n, 1), ph, pw, bpp), 0xA5, dtype=torch.uint8, device="cuda")     # (every byte must be overwritten)


def _pixels(raw, fmt):
    """(n, ph, pw, bpp) bytes -> an array shaped like S.expected's"""
    if fmt == "grey16":
        return raw.view("<u2")[..., 0]
    return raw if fmt == "rgb" else raw[..., 0]


def _read(call, q, pw, ph, fmt):
    """call(q, pw, ph, d_out, out_cap) -> (status, stats); -> (the tensor's bytes, status, stats)"""
    t = _tensor(len(q), ph, pw, _bpp(fmt))
    st, stats = call(q, pw, ph, t.data_ptr(), len(q) * ph * pw * _bpp(fmt))
    return t.cpu().numpy()[: len(q)], st, stats


def _files_call(mic, files, fmt):
    return lambda q, pw, ph, d, cap: mic.wsi_multi_read_patches(files, q, pw, ph, d, cap, **S.fmt_args(fmt))


def _want(levels, q, pw, ph):
    """the expected patches of q over the level images levels[slide][level]"""
    return [S.expected(levels[s][l], [(x, y)], pw, ph)[0] for x, y, s, l in q]


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_one_call_over_every_slide_and_level(mic, sets, fmt):
    """Every check of _one_call holds for each patch size; the plane modes are collected over the three sizes, as
    tests/test_gpu_wsi_patches.py collects them: the 1 x 1 patches of S.origins reach none of A's noise, white and black tiles."""
    seen = set()
    for pw, ph in M.PATCHES:
        seen |= _one_call(mic, sets[fmt], fmt, pw, ph)
    assert {2, 3} <= seen and (0 in seen or 1 in seen), seen            # constant, stream and raw planes were all read
    if fmt != "rgb":
        assert {0, 1} <= seen, seen


def _one_call(mic, st_, fmt, pw, ph):
    """one call over A, B, C and all their levels with pw x ph patches; -> the plane modes of the tiles it touched"""
    q = M.patch_list(st_["parsed"], pw, ph)
    assert len({(s, l) for _, _, s, l in q[:8]}) > 3                      # neighbours belong to different slides and levels
    raw, st, stats = _read(_files_call(mic, st_["files"], fmt), q, pw, ph, fmt)
    got = _pixels(raw, fmt)
    for i, want in enumerate(_want(st_["levels"], q, pw, ph)):
        assert np.array_equal(got[i], want), (q[i], pw, ph)
    assert (st == mic.MIC_OK).all()
    # byte-identical to the existing single-slide call, group by group
    old = np.zeros_like(raw)
    for s, level, xy in M.groups(st_["parsed"], pw, ph):
        t = _tensor(len(xy), ph, pw, _bpp(fmt))
        gst, _ = mic.wsi_read_patches(st_["files"][s], level, xy, pw, ph, t.data_ptr(), t.numel())
        assert (gst == mic.MIC_OK).all()
        part = t.cpu().numpy()
        left = {}
        for k, o in enumerate(xy):
            left.setdefault(o, []).append(k)
        for i, (x, y, fs, fl) in enumerate(q):
            if (fs, fl) == (s, level):
                old[i] = part[left[(x, y)][0]]
    assert raw.tobytes() == old.tobytes()
    slide_of, tile_of, pieces, fs = mic.wsi_multi_patch_plan(st_["files"], q, pw, ph, **S.fmt_args(fmt))
    assert stats["tiles_decoded"] == slide_of.size and stats["pieces"] == pieces and stats["slabs"] >= 1 and stats["slides_read"] == 3
    seen = set()
    for s, t in zip(slide_of.tolist(), tile_of.tolist()):
        seen.update(st_["parsed"][s].modes(t))
    return seen


def test_each_tile_is_decoded_once(mic, sets):
    st_ = sets["rgb"]
    q = [(3 + i % 10, 2 + i // 10, 0, 0) for i in range(100)] + [(2 + i % 5, 1 + i // 5, 1, 0) for i in range(100)]   # inside tile (0, 0) of A, of B
    raw, st, stats = _read(_files_call(mic, st_["files"], "rgb"), q, 24, 20, "rgb")
    assert stats["tiles_decoded"] == 2 and stats["pieces"] == 200 and stats["slides_read"] == 2 and (st == 0).all()
    for i, want in enumerate(_want(st_["levels"], q, 24, 20)):
        assert np.array_equal(raw[i], want), q[i]


class _CountingSource:
    def __init__(self, data):
        self.data, self.reads = data, []

    def __call__(self, off, n):
        self.reads.append((off, n))
        return self.data[off: off + n]


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_the_reader_door_gives_the_same_bytes_and_reads_touched_blobs_only(mic, sets, fmt):
    st_ = sets[fmt]
    a, b, c = st_["files"]
    files = [a, GARBAGE, b, c, a]                                          # slide 1 is named by no patch; slide 4 is slide 0 again
    parsed = [st_["parsed"][0], None, st_["parsed"][1], st_["parsed"][2], st_["parsed"][0]]
    pw, ph = 24, 20
    remap = {0: 0, 1: 2, 2: 3}
    q = [(x, y, remap[s], l) for x, y, s, l in M.patch_list(st_["parsed"], pw, ph)]
    q += [(x, y, 4, l) for x, y, s, l in q[:40] if s == 0]
    base, st0, stats0 = _read(_files_call(mic, files, fmt), q, pw, ph, fmt)
    srcs = [_CountingSource(d) for d in (a, b, b, c)]                      # (the unnamed reader: a good file that must not be read)
    rd = [mic.WsiReader(s, len(s.data)) for s in srcs]
    try:
        for s in srcs:
            s.reads.clear()
        readers = [rd[0], rd[1], rd[2], rd[3], rd[0]]
        got, st, stats = _read(lambda q_, w, h, d, cap: mic.wsi_readers_read_patches(readers, q_, w, h, d, cap, **S.fmt_args(fmt)), q, pw, ph, fmt)
        assert got.tobytes() == base.tobytes() and np.array_equal(st, st0) and stats == stats0 and (st == 0).all()
        assert srcs[1].reads == []
        slide_of, tile_of, _, _ = mic.wsi_multi_patch_plan(files, q, pw, ph, **S.fmt_args(fmt))
        for src, slides in ((srcs[0], (0, 4)), (srcs[2], (2,)), (srcs[3], (3,))):
            f = parsed[slides[0]]
            body = 48 + 20 * f.nlev + 16 * f.total
            offs = np.concatenate([[0], np.cumsum([len(x) for x in f.blobs])])
            want = np.zeros(len(src.data), dtype=np.int32)
            for s, t in zip(slide_of.tolist(), tile_of.tolist()):
                if s in slides:
                    want[body + offs[t]: body + offs[t + 1]] += 1
            fetched = np.zeros_like(want)
            for off, n in src.reads:
                fetched[off: off + n] += 1
            assert np.array_equal(fetched, want), slides
        # a missing reader no patch names is fine; one a patch names fails alone
        readers[1] = None
        got, st, stats = _read(lambda q_, w, h, d, cap: mic.wsi_readers_read_patches(readers, q_, w, h, d, cap, **S.fmt_args(fmt)), q, pw, ph, fmt)
        assert got.tobytes() == base.tobytes() and (st == 0).all()
        got, st, stats = _read(lambda q_, w, h, d, cap: mic.wsi_readers_read_patches(readers, q_, w, h, d, cap, **S.fmt_args(fmt)),
                               q + [(0, 0, 1, 0)], pw, ph, fmt)
        assert got[: len(q)].tobytes() == base.tobytes() and (st[:-1] == 0).all() and st[-1] == mic.MIC_ERR_ARGS and not got[-1].any()
    finally:
        for r in rd:
            r.close()


def _spanning(parsed):
    """24 x 20 patches on a grid over level 0 of A, B and C: every level-0 tile of the three slides"""
    q = []
    for s, f in enumerate(parsed):
        lw, lh = f.levels[0][:2]
        q += [(x, y, s, 0) for y in range(-5, lh, 17) for x in range(-5, lw, 19)]
    return q


def test_slabs_under_a_small_workspace(mic, sets):
    """A child process with an 8 MB workspace ceiling: a sub-batch of the unit codec then holds a handful of tiles (six 64 x 64 RGB
    tiles: tests/test_gpu_wsi_patches.py), so the 27 level-0 tiles of A, B and C take several sub-batches, whose cuts fall between
    slides of different tile sizes.  The bytes must be those of the unconstrained call."""
    st_ = sets["rgb"]
    q = _spanning(st_["parsed"])
    want, st, stats = _read(_files_call(mic, st_["files"], "rgb"), q, 24, 20, "rgb")
    assert stats["tiles_decoded"] == 27 and (st == 0).all()
    for i, w in enumerate(_want(st_["levels"], q, 24, 20)):
        assert np.array_equal(want[i], w), q[i]
    code = r'''
import sys, hashlib, numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import __graft_entry__ as e
mic = e.load_package()
import wsi_multi_slides as M
files = [M.device_file(mic, name, "rgb") for name in M.NAMES]
q = %r
t = torch.full((len(q), 20, 24, 3), 0xA5, dtype=torch.uint8, device="cuda")
st, stats = mic.wsi_multi_read_patches(files, q, 24, 20, t.data_ptr(), t.numel())
assert (st == 0).all() and stats["tiles_decoded"] == 27 and stats["slabs"] >= 2, stats
# Sub-batches whose largest pieces differ (the gather's grid y follows the largest piece of each sub-batch): patches of 65 x 64 over
# B, C and a slide of 128 x 128 tiles.  The first patch touches the first unit, B's tile 0, in its corner pixel alone; C's nine
# 16 x 16 tiles follow; the last patch lies wholly inside the last unit, the slide's tile 3 -- a 65 x 64 piece, two row chunks.
yy, xx = np.mgrid[0:256, 0:256]
ramp = (3 * xx + 2 * yy) // 2 + np.random.default_rng(13).integers(0, 4, (256, 256))
big = np.stack([ramp %% 256, (ramp // 2 + 40) %% 256, (255 - ramp) %% 256], -1).astype(np.uint8)
files2 = [files[1], files[2], mic.compress_wsi(big, 256, 256, tile_w=128, tile_h=128, levels=1)]
whole = [mic.decompress_wsi_level(f, 0) for f in files2]
assert np.array_equal(whole[2], big)
q2 = [(-64, -63, 0, 0), (0, 0, 1, 0), (130, 130, 2, 0)]
slide_of, tile_of, pieces, fs = mic.wsi_multi_patch_plan(files2, q2, 65, 64)
assert slide_of.tolist() == [0] + [1] * 9 + [2] and tile_of.tolist()[0] == 0 and tile_of.tolist()[-1] == 3 and pieces == 11
t2 = torch.full((len(q2), 64, 65, 3), 0xA5, dtype=torch.uint8, device="cuda")
st, stats = mic.wsi_multi_read_patches(files2, q2, 65, 64, t2.data_ptr(), t2.numel())
assert (st == 0).all() and stats["tiles_decoded"] == 11 and stats["slabs"] >= 2, stats
got = t2.cpu().numpy()
for i, (x, y, s, l) in enumerate(q2):
    assert np.array_equal(got[i], M.S.expected(whole[s], [(x, y)], 65, 64)[0]), q2[i]
assert np.count_nonzero(got[0].any(-1)) <= 1 and np.array_equal(got[0, 63, 64], whole[0][0, 0]) and np.array_equal(got[2], big[130:194, 130:195])
print("ok", hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest())
''' % (ROOT, os.path.join(ROOT, "tests"), q)
    env = dict(os.environ, MIC_HIP_WS_BUDGET_MB="8")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ("ok " + hashlib.sha256(np.ascontiguousarray(want).tobytes()).hexdigest()) in r.stdout, r.stdout + r.stderr


def _code(mic, call):
    try:
        call()
    except mic.MicError as e:
        return e.code
    return mic.MIC_OK


@pytest.mark.parametrize("fmt", ["rgb", "grey16"])
def test_failures_stay_local(mic, sets, fmt):
    st_ = sets[fmt]
    pw, ph = 24, 20
    # slide B with the first plane of its level-0 tile 1 damaged (a mode byte no decoder knows)
    f = S.Mic3File(st_["files"][1])
    tile = 1
    off, _ = f.plane_spans(tile)[0]
    assert f.blobs[tile][off] == 2
    f.blobs[tile][off] = 9
    bad_b = f.bytes()
    tw, th = M.tile_size(f)
    code = _code(mic, lambda: mic.decompress_wsi_tile(bad_b, 0, tile % f.levels[0][2], tile // f.levels[0][2]))
    assert code == mic.MIC_ERR_CORRUPT
    other = sets[M.OTHER_FORMAT[fmt]]["files"][1]                          # slide D
    files = [st_["files"][0], bad_b, GARBAGE, other, st_["files"][2]]
    levels = [st_["levels"][0], st_["levels"][1], None, None, st_["levels"][2]]
    remap = {0: 0, 1: 1, 2: 4}
    q = [(x, y, remap[s], l) for x, y, s, l in M.patch_list(st_["parsed"], pw, ph)]
    q += [(0, 0, 2, 0), (5, 5, 2, 1), (0, 0, 3, 0), (10, 10, 3, 1)]          # the garbage slide, the slide of another format
    q += [(0, 0, 0, S.LEVELS), (0, 0, 4, -1), (3, 3, 1, 2)]                  # levels their slides do not have
    order = np.random.default_rng(3).permutation(len(q))
    q = [q[i] for i in order]
    t = _tensor(1, ph, pw, _bpp(fmt))
    garbage_code = _code(mic, lambda: mic.wsi_read_patches(GARBAGE, 0, [(0, 0)], pw, ph, t.data_ptr(), t.numel()))
    assert garbage_code == mic.MIC_ERR_CORRUPT
    raw, st, stats = _read(_files_call(mic, files, fmt), q, pw, ph, fmt)
    got = _pixels(raw, fmt)
    assert stats["slides_read"] == 3
    lw, lh = f.levels[0][:2]
    hit = 0
    for i, (x, y, s, l) in enumerate(q):
        if s == 2:
            assert st[i] == garbage_code and not raw[i].any(), q[i]
        elif s == 3:
            assert st[i] == mic.MIC_ERR_ARGS and not raw[i].any(), q[i]
        elif not 0 <= l < len(levels[s]):
            assert st[i] == mic.MIC_ERR_ARGS and not raw[i].any(), q[i]
        else:
            touches = s == 1 and l == 0 and tile in mic.wsi_patch_plan(lw, lh, tw, th, [(x, y)], pw, ph)[0]
            hit += touches
            assert st[i] == (code if touches else mic.MIC_OK), (q[i], st[i])
            if not touches:
                assert np.array_equal(got[i], S.expected(levels[s][l], [(x, y)], pw, ph)[0]), q[i]
    assert hit > 0


def test_argument_errors_come_back_before_any_launch(mic, sets):
    st_ = sets["rgb"]
    files = st_["files"]
    t = _tensor(2, 20, 24, 3)
    q = [(0, 0, 0, 0), (10, 10, 1, 1)]
    cap = 2 * 20 * 24 * 3
    rd = [mic.WsiReader(d) for d in files]
    doors = [lambda q_, w, h, d, c, **kw: mic.wsi_multi_read_patches(files, q_, w, h, d, c, **kw),
             lambda q_, w, h, d, c, **kw: mic.wsi_readers_read_patches(rd, q_, w, h, d, c, **kw)]
    try:
        for door in doors:
            for args, kw, want in [((q, 0, 20, t.data_ptr(), cap), {}, mic.MIC_ERR_ARGS), ((q, 24, -1, t.data_ptr(), cap), {}, mic.MIC_ERR_ARGS),
                                   ((q, 24, 20, t.data_ptr(), cap - 1), {}, mic.MIC_ERR_CAPACITY),
                                   ((q, 24, 20, t.data_ptr(), cap), dict(channels=2), mic.MIC_ERR_UNSUPPORTED),
                                   ((q, 24, 20, t.data_ptr(), cap), dict(bits_per_sample=16), mic.MIC_ERR_UNSUPPORTED),
                                   ((q, 0, 20, t.data_ptr(), cap), dict(channels=2), mic.MIC_ERR_ARGS),       # (the order the header states)
                                   ((q, 24, 20, t.data_ptr(), 0), dict(channels=2), mic.MIC_ERR_UNSUPPORTED),
                                   ((q + [(0, 0, 3, 0)], 24, 20, t.data_ptr(), 2 * cap), {}, mic.MIC_ERR_ARGS),
                                   ((q + [(0, 0, -1, 0)], 24, 20, t.data_ptr(), 2 * cap), {}, mic.MIC_ERR_ARGS),
                                   ((q, 24, 20, 0, cap), {}, mic.MIC_ERR_ARGS)]:
                with pytest.raises(mic.MicError) as e:
                    door(*args, **kw)
                assert e.value.code == want, (args, kw)
            st, stats = door([], 24, 20, t.data_ptr(), 0)                   # n = 0: nothing to do, and that is no error
            assert st.size == 0 and stats == dict(tiles_decoded=0, pieces=0, slabs=0, slides_read=0)
        host = np.zeros(cap, dtype=np.uint8)                               # pageable host memory is no place for the tensor
        with pytest.raises(mic.MicError) as e:
            doors[0](q, 24, 20, host.ctypes.data, cap)
        assert e.value.code == mic.MIC_ERR_ARGS
        assert (t.cpu().numpy() == 0xA5).all()                            # none of these calls wrote a byte
        st, stats = doors[0](q, 24, 20, t.data_ptr(), cap)                # ... and the tensor was a good one
        assert (st == 0).all()
        want = _want(st_["levels"], q, 24, 20)
        assert np.array_equal(t.cpu().numpy()[0], want[0]) and np.array_equal(t.cpu().numpy()[1], want[1])
    finally:
        for r in rd:
            r.close()


@pytest.mark.parametrize("fmt", ["rgb", "grey16"])
def test_pinned_host_memory_receives_the_same_bytes(mic, sets, fmt):
    st_ = sets[fmt]
    pw, ph = 71, 37
    q = M.patch_list(st_["parsed"], pw, ph)
    base, st0, stats0 = _read(_files_call(mic, st_["files"], fmt), q, pw, ph, fmt)
    n = len(q) * ph * pw * _bpp(fmt)
    host = mic.host_alloc(n)
    try:
        host[:] = 0xA5
        st, stats = mic.wsi_multi_read_patches(st_["files"], q, pw, ph, host.ctypes.data, n, **S.fmt_args(fmt))
        assert (st == 0).all() and stats == stats0 and host.tobytes() == base.tobytes()
    finally:
        mic.host_free(host)
