"""The frame cache of the MIC2 crop readers on the device (csrc/mic_mic2_crops.hip: mic_hip_mic2_reader_set_cache,
mic2_cached_read_crops, k_mic2_accumulate_frames).  The codec is lossless: the expected value of every crop is the stack of
decompress_multi_frame, padded with zeros and cropped in numpy (mic2_crop_volumes.expected); what the cache does -- outcomes,
anchors, the streams decoded, residency, counters -- is the host model's (mic2_frame_cache_model.py)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT
import mic2_crop_volumes as V
import mic2_frame_cache_model as FM
import mic2_frame_cache_volumes as FV
import mic2_multi_volumes as M
import out_spec_ref as R

pytestmark = pytest.mark.gpu

CROP = (11, 9, 3)          # cw, ch, cd of the parity lists: wider than the 8-pixel frame, odd row pitch


@pytest.fixture(scope="module")
def volumes(mic, gpu_ready):
    return {name: FV.make_files(mic, name) for name in FV.SIZES}


def _origins(w, h, n):
    """inside; negative and overhanging origins in x, y and z; wholly outside: names frames 0 .. 3, n - 2, n - 1"""
    return [(-4, -2, 1), (w - 5, h - 4, -1), (2, 3, n - 2), (1, 1, 1), (w, 0, 0), (0, 0, n)]


def _check(got, want, where):
    for i in range(len(want)):
        assert np.array_equal(got[i], want[i]), (where, i)


def _typed(mic, vol, xyz, cw, ch, cd):
    """(spec, expected bits) of an f32 tensor with slope and intercept"""
    a, b = R.PAIRS[0]
    spec = mic.OutSpec("f32", affine=[(a, b)], pad=-3.0)
    want = R.convert(V.expected(vol, xyz, cw, ch, cd), "f32", a, b, pad=-3.0, outside=FV.outside(vol, xyz, cw, ch, cd))
    R.assert_no_subnormals(want, "f32")
    return spec, want


def _read(rd, xyz, cw, ch, cd, spec=None):
    """(samples or bits, status, stats) of rd.read_crops"""
    if spec is None:
        return FV.read_native(lambda *a: rd.read_crops(*a), xyz, cw, ch, cd)
    buf = R.Buffer(len(xyz) * cd * ch * cw, spec.dtype)
    st, stats = rd.read_crops(xyz, cw, ch, cd, buf.ptr, buf.nbytes, spec=spec)
    return buf.bits().reshape(len(xyz), cd, ch, cw), st, stats


@pytest.mark.parametrize("typed", [False, True])
@pytest.mark.parametrize("temporal", [False, True])
@pytest.mark.parametrize("name", sorted(FV.SIZES))
def test_parity_cold_warm_and_after_eviction(mic, volumes, name, temporal, typed):
    vol, data = volumes[name]["vol"], volumes[name]["files"][temporal]
    n, h, w = vol.shape
    cw, ch, cd = CROP
    xyz = _origins(w, h, n)
    named = FV.named_frames(w, h, n, xyz, cw, ch, cd)
    assert named == [0, 1, 2, 3, n - 2, n - 1]
    spec, want = _typed(mic, vol, xyz, cw, ch, cd) if typed else (None, V.expected(vol, xyz, cw, ch, cd))
    other = FV.at_frames([5, 6, 7], x=-3, y=h - 4)                        # three misses: half of the six go
    want_other = V.expected(vol, other, cw, ch, 1)
    with mic.Mic2Reader(data) as rd, mic.FrameCache(w, h, len(named)) as cache:
        rd.set_cache(cache)
        got, st, stats = _read(rd, xyz, cw, ch, cd, spec)
        _check(got, want, "cold")
        assert (st == 0).all() and stats["frames_decoded"] == (n if temporal else len(named)) and stats["slabs"] == 1
        assert rd.cache_probe(np.arange(n)).nonzero()[0].tolist() == named
        got, st, stats = _read(rd, xyz, cw, ch, cd, spec)
        _check(got, want, "warm")
        assert (st == 0).all() and stats["frames_decoded"] == 0 and stats["slabs"] == 0
        got, st, stats = FV.read_native(lambda *a: rd.read_crops(*a), other, cw, ch, 1)
        _check(got, want_other, "evicting")
        assert (st == 0).all() and stats["frames_decoded"] == (4 if temporal else 3)      # temporal: behind frame 3
        assert rd.cache_probe(np.arange(n)).nonzero()[0].tolist() == [3, 5, 6, 7, n - 2, n - 1]
        got, st, stats = _read(rd, xyz, cw, ch, cd, spec)
        _check(got, want, "after eviction")
        assert (st == 0).all() and stats["frames_decoded"] == 3 and stats["slabs"] == 1   # frames 0, 1, 2, from frame 0's stream
        cache.clear()
        assert not rd.cache_probe(np.arange(n)).any()
        got, st, stats = _read(rd, xyz, cw, ch, cd, spec)
        _check(got, want, "after clear")
        assert (st == 0).all() and stats["frames_decoded"] == (n if temporal else len(named))
        assert cache.stats()["device_bytes"] == len(named) * mic.frame_cache_slot_bytes(w, h)
        rd.set_cache(None)


def _union(m, frames):
    c = np.zeros(len(m.data), dtype=bool)
    for f in frames:
        b, e = m.span(f)
        c[b:e] = True
    return c


def test_work_really_is_skipped(mic, volumes):
    vol = volumes["wave"]["vol"]
    n, h, w = vol.shape
    cw, ch = 20, 10
    for temporal in (False, True):
        data = volumes["wave"]["files"][temporal]
        m, src = V.Mic2File(data), V.RecordingSource(data)
        with mic.Mic2Reader(src, len(data)) as rd, mic.FrameCache(w, h, 4) as cache:
            rd.set_cache(cache)
            src.reads.clear()
            nine = [(5, 5, 9)]
            got, st, stats = _read(rd, nine, cw, ch, 1)
            _check(got, V.expected(vol, nine, cw, ch, 1), "cold")
            assert stats["frames_decoded"] == (10 if temporal else 1)
            assert np.array_equal(src.coverage() > 0, _union(m, range(10) if temporal else [9]))
            assert rd.cache_probe(np.arange(n)).nonzero()[0].tolist() == [9]
            src.reads.clear()
            got, st, stats = _read(rd, nine + [(40, 20, 9)], cw, ch, 1)   # fresh origins, the same frame
            _check(got, V.expected(vol, nine + [(40, 20, 9)], cw, ch, 1), "warm")
            assert src.reads == [] and stats["frames_decoded"] == 0 and stats["slabs"] == 0 and (st == 0).all()
            # frame 9 is resident: frames 11 .. 12 of a temporal file need the residuals of frames 10, 11 and 12 and nothing else
            far = [(7, 3, 11)]
            got, st, stats = _read(rd, far, cw, ch, 2)
            _check(got, V.expected(vol, far, cw, ch, 2), "anchored")
            if temporal:
                b, e = m.span(10)[0], m.span(12)[1]
                assert src.reads == [(b, e - b)] and stats["frames_decoded"] == 3 and stats["slabs"] == 1
            else:
                assert np.array_equal(src.coverage() > 0, _union(m, [11, 12])) and stats["frames_decoded"] == 2
            assert rd.cache_probe(np.arange(n)).nonzero()[0].tolist() == [9, 11, 12]
            rd.set_cache(None)


def _expect_model(rd, cache, model, res, n):
    assert set(rd.cache_probe(np.arange(n)).nonzero()[0].tolist()) == {k & 0xFFFFFFFF for k in res["resident"]}
    st = cache.stats()
    assert {k: st[k] for k in model.counters} == model.counters, (st, model.counters)
    assert st["resident"] == len(res["resident"])


@pytest.mark.parametrize("temporal", [False, True])
def test_counters_and_probe_follow_the_model(mic, volumes, temporal):
    vol, data = volumes["odd"]["vol"], volumes["odd"]["files"][temporal]
    n, h, w = vol.shape
    cw, ch = 9, 7
    # calls of four frames each; slots = call size - 1, = call size, 1 and 0 cross every capacity seam
    trace = [[2, 5, 9, 12], [2, 5, 9, 12], [3, 6, 9, 11], [0, 5, 7, 12], [12], [1, 2, 3, 4]]
    for nslots in (3, 4, 1, 0):
        model = FM.FrameCacheModel(nslots, [(n, temporal)])
        with mic.Mic2Reader(data) as rd, mic.FrameCache(w, h, nslots) as cache:
            rd.set_cache(cache)
            for k, frames in enumerate(trace):
                xyz = FV.at_frames(frames, x=-2, y=4)
                res = model.call([(0, frames)])
                got, st, stats = _read(rd, xyz, cw, ch, 1)
                _check(got, V.expected(vol, xyz, cw, ch, 1), (nslots, k))
                assert (st == 0).all() and stats["frames_decoded"] == len(res["decoded"]), (nslots, k, stats, sorted(res["decoded"]))
                assert stats["slabs"] == (1 if res["decoded"] else 0) and stats["pieces"] == len(frames)
                _expect_model(rd, cache, model, res, n)
            rd.set_cache(None)
            assert cache.stats()["resident"] == 0                         # detaching drops the reader's entries


def _budget_mb(mic, w, h, n):
    """a workspace ceiling, in MiB, under which the n frames are cut into sub-batches of 2 .. 5 (mic2_batch_plan: the cut rule)"""
    for mb in range(1, 64):
        cuts, _ = mic.mic2_batch_plan([(w, h, n)], mb << 20)
        if 2 <= int(cuts[1]) <= 5:
            return mb, int(cuts[1])
    raise AssertionError("no such budget")


def test_sub_batch_seams_under_a_small_workspace(mic):
    """tests/mic2_frame_cache_chunking_check.py in a fresh process whose workspace ceiling cuts a temporal run of 16 frames of
    64 x 33 at least twice: the whole-frame sum's carry crosses the seams in the session's workspace"""
    w, h, n = FV.SIZES["wave"]
    mb, per = _budget_mb(mic, w, h, n)
    assert -(-n // per) >= 3
    env = dict(os.environ, MIC_HIP_WS_BUDGET_MB=str(mb))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mic2_frame_cache_chunking_check.py")], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "mic2 frame cache seams ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("temporal", [False, True])
def test_a_damaged_frame(mic, volumes, temporal):
    vol = volumes["wave"]["vol"]
    n, h, w = vol.shape
    cw, ch = 20, 10
    bad = FV.damaged(mic, "wave", temporal, 5)
    frames = [3, 5, 6, 8]
    xyz = FV.at_frames(frames)
    xyzv = [c + (0,) for c in xyz]
    want = V.expected(vol, xyz, cw, ch, 1)
    with mic.Mic2Reader(bad) as plain:                                    # today's codes: the same door without a cache
        _, st0, bad0, _ = FV.read_native(lambda *a: mic.mic2_readers_read_crops([plain], *a), xyzv, cw, ch, 1)
    lost = [5, 6, 8] if temporal else [5]
    assert [f for f, s in zip(frames, st0) if s != 0] == lost and len({int(s) for s in st0 if s != 0}) == 1
    model = FM.FrameCacheModel(8, [(n, temporal)])
    with mic.Mic2Reader(bad) as rd, mic.FrameCache(w, h, 8) as cache:
        rd.set_cache(cache)
        res = model.call([(0, frames)], bad=[(0, 5)])
        assert sorted(f for (_, f) in res["failed"]) == lost
        got, st, badf, stats = FV.read_native(lambda *a: mic.mic2_readers_read_crops([rd], *a), xyzv, cw, ch, 1)
        assert st.tolist() == st0.tolist() and badf.tolist() == bad0.tolist()
        assert [int(b) for b, s in zip(badf, st) if s != 0] == [5] * len(lost)
        _check(got[:1], want[:1], "in front of the damage")
        if not temporal:
            _check(got[2:], want[2:], "behind the damaged frame")
        _expect_model(rd, cache, model, res, n)
        assert rd.cache_probe(frames).tolist() == [f not in lost for f in frames]
        # the frames below the damage are resident and right: frame 4 is summed from frame 3 (a temporal file), frame 3 hits
        nxt = FV.at_frames([3, 4], x=10, y=1)
        res = model.call([(0, [3, 4])])
        got, st, stats = _read(rd, nxt, cw, ch, 1)
        _check(got, V.expected(vol, nxt, cw, ch, 1), "the next call")
        assert (st == 0).all() and stats["frames_decoded"] == 1
        _expect_model(rd, cache, model, res, n)
        rd.set_cache(None)


class _Flaky:
    """a source that fails on demand"""

    def __init__(self, data):
        self.data, self.fail = bytes(data), False

    def __call__(self, off, n):
        if self.fail:
            raise IOError("the source is gone")
        return self.data[off: off + n]


@pytest.mark.parametrize("temporal", [False, True])
def test_a_failing_callback_undoes_the_call(mic, volumes, temporal):
    vol, data = volumes["odd"]["vol"], volumes["odd"]["files"][temporal]
    n, h, w = vol.shape
    cw, ch = 9, 7
    src = _Flaky(data)
    with mic.Mic2Reader(src, len(data)) as rd, mic.FrameCache(w, h, 3) as cache:
        rd.set_cache(cache)
        first = FV.at_frames([2, 4, 6])
        got, st, stats = _read(rd, first, cw, ch, 1)
        before, probe = cache.stats(), rd.cache_probe(np.arange(n)).tolist()
        src.fail = True
        with pytest.raises(Exception):
            _read(rd, FV.at_frames([4, 8, 9]), cw, ch, 1)                 # a hit, two misses that evict
        src.fail = False
        assert cache.stats() == before and rd.cache_probe(np.arange(n)).tolist() == probe
        nxt = FV.at_frames([2, 4, 6, 8])
        got, st, stats = _read(rd, nxt, cw, ch, 1)
        _check(got, V.expected(vol, nxt, cw, ch, 1), "the next good call")
        assert (st == 0).all() and stats["frames_decoded"] == (2 if temporal else 1)       # frames 7 and 8 behind frame 6
        after = cache.stats()                                             # three hits fill the three slots: frame 8 is bypassed
        assert (after["hits"], after["misses"], after["bypassed"], after["evictions"], after["calls"]) == \
            (before["hits"] + 3, before["misses"], before["bypassed"] + 1, before["evictions"], before["calls"] + 1)
        rd.set_cache(None)


def test_many_readers_in_one_call(mic, volumes):
    wave, odd = volumes["wave"], volumes["odd"]
    n, h, w = wave["vol"].shape
    no, ho, wo = odd["vol"].shape
    cw, ch, cd = 12, 8, 2
    with mic.Mic2Reader(wave["files"][False]) as r_ind, mic.Mic2Reader(wave["files"][True]) as r_tmp, \
            mic.Mic2Reader(odd["files"][True]) as r_none, mic.FrameCache(w, h, 6) as cache:
        r_ind.set_cache(cache)
        r_tmp.set_cache(cache)
        readers = [r_ind, r_tmp, r_none, r_tmp]                           # the temporal reader is volumes 1 and 3
        vols = [wave["vol"], wave["vol"], odd["vol"], wave["vol"]]
        per = [[(3, 2, 4), (-2, 30, 9)], [(50, -1, 6)], [(30, 10, 3), (0, 0, no - 1)], [(10, 10, 7), (1, 1, 12)]]
        xyzv = M.interleave(per)
        want = M.expected_multi(vols, xyzv, cw, ch, cd)
        calls = [[(0, [4, 5, 9, 10]), (1, [6, 7, 8, 12, 13])]] * 2
        model = FM.FrameCacheModel(6, [(n, False), (n, True)])
        for k, call in enumerate(calls):
            res = model.call(call)
            got, st, badf, stats = FV.read_native(lambda *a: mic.mic2_readers_read_crops(readers, *a), xyzv, cw, ch, cd)
            _check(got, want, k)
            assert (st == 0).all() and (badf == -1).all()
            assert stats["frames_decoded"] == len(res["decoded"]) + no and stats["volumes_read"] == 4   # the reader without a cache: frames 0 .. last
            cs = cache.stats()
            assert {c: cs[c] for c in model.counters} == model.counters, (k, cs, model.counters)
            assert set(r_ind.cache_probe(np.arange(n)).nonzero()[0].tolist()) == {x & 0xFFFFFFFF for x in res["resident"] if x >> 32 == 0}
            assert set(r_tmp.cache_probe(np.arange(n)).nonzero()[0].tolist()) == {x & 0xFFFFFFFF for x in res["resident"] if x >> 32 == 1}
        assert model.counters["bypassed"] > 0 and model.counters["hits"] > 0              # nine keys, six slots
        # each reader a cache of its own; the one of another frame size serves the third
        with mic.FrameCache(wo, ho, 4) as small:
            r_none.set_cache(small)
            for k in range(2):
                res = model.call(calls[0])
                got, st, badf, stats = FV.read_native(lambda *a: mic.mic2_readers_read_crops(readers, *a), xyzv, cw, ch, cd)
                _check(got, want, ("two caches", k))
                assert stats["frames_decoded"] == len(res["decoded"]) + (no if k == 0 else 0)   # its frames 3, 4 and 12: cold from frame 0 on, then hits
            assert small.stats()["hits"] == 3 and small.stats()["misses"] == 3
            r_none.set_cache(None)
        r_ind.set_cache(None)
        r_tmp.set_cache(None)


def test_two_threads_share_one_cache(mic, volumes):
    vol = volumes["wave"]["vol"]
    n, h, w = vol.shape
    cw, ch = 16, 12
    lists = [[FV.at_frames(fr, x=1 + t, y=2) for fr in ([1, 4, 7], [4, 7, 10], [2, 3], [10, 11, 12, 13], [1, 4, 7])] for t in range(2)]
    errors, keys = [], [0, 0]
    with mic.FrameCache(w, h, 5) as cache:
        readers = [mic.Mic2Reader(volumes["wave"]["files"][bool(t)]) for t in range(2)]
        for rd in readers:
            rd.set_cache(cache)

        def work(t):
            try:
                for _ in range(3):
                    for xyz in lists[t]:
                        got, st, stats = _read(readers[t], xyz, cw, ch, 1)
                        _check(got, V.expected(vol, xyz, cw, ch, 1), t)
                        assert (st == 0).all()
                        keys[t] += len(xyz)
            except Exception as e:                                        # (reported by the main thread)
                errors.append(e)
        threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        st = cache.stats()
        assert st["hits"] + st["misses"] + st["bypassed"] == sum(keys) and st["calls"] == 30
        for rd in readers:
            rd.close()
        assert cache.stats()["resident"] == 0


@pytest.mark.parametrize("temporal", [False, True])
def test_no_cache_nothing_new(mic, volumes, temporal):
    vol, data = volumes["wave"]["vol"], volumes["wave"]["files"][temporal]
    n, h, w = vol.shape
    cw, ch, cd = CROP
    xyz = _origins(w, h, n)
    want = V.expected(vol, xyz, cw, ch, cd)
    with mic.Mic2Reader(data) as rd, mic.FrameCache(w, h, 4) as cache:
        ref, st0, stats0 = FV.read_native(lambda *a: mic.mic2_read_crops(data, *a), xyz, cw, ch, cd)
        rd.set_timing(True)
        got, st, stats = _read(rd, xyz, cw, ch, cd)
        names = [k for k, _ in rd.last_timings()]
        assert np.array_equal(got, ref) and np.array_equal(ref, want) and st.tolist() == st0.tolist() and stats == stats0
        assert "k_mic2_accumulate_frames" not in names and "k_mic2_gather_cached" not in names and "k_mic2_cache_fill" not in names
        assert ("k_mic2_accumulate_crops" if temporal else "k_mic2_gather_crops") in names
        # attached, the same call runs the new kernels; detached again, the old ones
        rd.set_cache(cache)
        got, st, stats = _read(rd, xyz, cw, ch, cd)
        names = [k for k, _ in rd.last_timings()]
        assert np.array_equal(got, want) and ("k_mic2_accumulate_frames" if temporal else "k_mic2_cache_fill") in names and "k_mic2_gather_cached" in names
        rd.set_cache(None)
        got, st, stats = _read(rd, xyz, cw, ch, cd)
        assert np.array_equal(got, ref) and stats == stats0 and "k_mic2_accumulate_frames" not in [k for k, _ in rd.last_timings()]


def test_set_cache_checks_the_format(mic, volumes):
    data = volumes["wave"]["files"][True]
    vol = volumes["wave"]["vol"]
    n, h, w = vol.shape
    rd = mic.Mic2Reader(data)
    for cwid, chei in ((w + 1, h), (w, h - 1), (h, w)):
        with mic.FrameCache(cwid, chei, 2) as c:
            with pytest.raises(mic.MicError) as e:
                rd.set_cache(c)
            assert e.value.code == mic.MIC_ERR_ARGS
    cache = mic.FrameCache(w, h, 2)
    rd.set_cache(cache)
    xyz = FV.at_frames([1, 2])
    got, st, stats = _read(rd, xyz, 8, 8, 1)
    _check(got, V.expected(vol, xyz, 8, 8, 1), "attached")
    assert cache.stats()["resident"] == 2
    with pytest.raises(mic.MicError) as e:
        cache.close()                                                     # attached: nothing is freed
    assert e.value.code == mic.MIC_ERR_ARGS
    got, st, stats = _read(rd, xyz, 8, 8, 1)
    assert stats["frames_decoded"] == 0 and np.array_equal(got, V.expected(vol, xyz, 8, 8, 1))
    rd.close()                                                            # close detaches
    assert cache.stats()["resident"] == 0
    cache.close()
