"""The two instances of the table kernels (csrc/mic_tables.hip: TbLds) on both sides of the line between them.

k_enc_tables_wg and k_dec_tables_wg come as a compact instance -- tANS units of at most 4096 symbols and tableLog <= 13, two
work-groups per CU -- and the standard one for everything else and for what the compact one was not launched for.  Launched
together, each leaves the other's units alone; MicUnit.tb_inst (mic_hip_debug_tab_inst) says which one built a unit's tables.  The class is decided on the device
(the alphabet is known after the histogram scan or the header parse), so the cases here sit on both sides of every term of it:

    largest symbol 4094, 4095 (the last of the compact class), 4096 and 8191, each at tableLog 12, 13 and 14 (req_tl, and a token
    count that lets optimal_table_log keep it); a -1 count at the top of the alphabet; a symbol of more than sixteen slots
    (tp_build's bitmap ranking, whose per-wave words the compact carve-up keeps); an rANS unit of a small alphabet (standard).

Bare FSE units (mode 1) run side by side through the debug doors of tests/table_doors.py; two small frame strips run through the
ordinary Session calls.  Every unit's bytes are the oracle's, its symbols come back from the decode, its tb_route is what the model of
tests/table_routes.py names and its tb_inst what the class rule above gives, on the encode and on the decode side.  One batch mixes
the classes; one holds 600 units of 4096 tokens -- on 256 CUs with two groups each more than one resident round, so that groups of
a later round start beside groups that are in the middle of their unit.  Both run twice on one session with identical bytes."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import table_doors as D
import table_routes as M

pytestmark = pytest.mark.gpu

STD, C4K = 1, 2                            # MIC_TBI_* (csrc/mic_dev.h)
C4K_SYMS, C4K_TL = 4096, 13

Case = namedtuple("Case", "name hist flavour req_tl tl")


def _inst(u):
    """the instance the class rule gives a unit the model has normalised"""
    return C4K if u.symbol_len <= C4K_SYMS and u.tl <= C4K_TL and u.flavour != 108 else STD


def _hist(top, n, low_top):
    """300 symbols that fall off geometrically (the first of them take hundreds of slots), a thin tail, and the largest symbol `top`;
    low_top: the three largest symbols occur once -- counts of -1 at the top of the alphabet"""
    h = np.zeros(top + 1, np.int64)
    body = np.exp(-np.arange(300) / 45.0)
    h[:300] = np.maximum(np.round(body / body.sum() * (n - 400)).astype(np.int64), 2)
    h[300:top - 8:max(1, (top - 308) // 120)] += 2
    h[top - 2:] = 1 if low_top else 9
    h[0] += n - h.sum()
    assert h.sum() == n and h[0] > 0 and h[top] > 0
    return h


def _cases():
    out = []
    for top in (4094, 4095, 4096, 8191):
        for tl, n in ((12, 30000), (13, 60000), (14, 100000)):
            out.append(Case(f"top{top}/tl{tl}", _hist(top, n, low_top=(tl == 13)), 2, tl, tl))
    out.append(Case("top4095/tl13/four-states", _hist(4095, 60000, False), 4, 13, 13))
    out.append(Case("top299/rans", _hist(299, 60000, False), 108, 13, 13))
    out.append(Case("top299/tl9", _hist(299, 4096, False), 2, 0, 9))
    return out


CASES = _cases()
_SYM, _UNIT, _REF = {}, {}, {}


def _symbols(c):
    if c.name not in _SYM:
        from conftest import load_package
        load_package()
        import importlib
        hash_u64 = importlib.import_module("medical_image_codec_amd.synth").hash_u64
        sym = np.repeat(np.arange(c.hist.size), c.hist).astype(np.uint16)
        _SYM[c.name] = sym[np.argsort(hash_u64(sym.size, 7), kind="stable")]
    return _SYM[c.name]


def _unit(c):
    if c.name not in _UNIT:
        _UNIT[c.name] = M.Unit(c.hist, c.flavour, c.req_tl)
    return _UNIT[c.name]


def _blob(mico, c):
    if c.name not in _REF:
        rc, blob = mico.fse_compress_tl(_symbols(c), c.flavour, c.req_tl)
        assert rc == 0, (c.name, rc)
        _REF[c.name] = blob
    return _REF[c.name]


def _tab_inst(mic, sess, i):
    r = C.c_uint32()
    L = mic.lib()
    L.mic_hip_debug_tab_inst.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    assert L.mic_hip_debug_tab_inst(sess._h, i, C.byref(r)) == 0
    return int(r.value)


def test_the_cases_sit_on_both_sides_of_the_class_line():
    """on the CPU, in front of every GPU run: the model gives each case the tableLog it is named for, the alphabets straddle 4096,
    the tableLogs straddle 13, and the two seams tp_build and the spread have in the compact carve-up are there"""
    seen = set()
    for c in CASES:
        u = _unit(c)
        assert u.rc == 0 and u.tl == c.tl and u.symbol_len == c.hist.size, (c.name, u.rc, u.tl, u.symbol_len)
        seen.add((u.symbol_len, u.tl, _inst(u)))
    for tl in (12, 13):
        assert {(4095, tl, C4K), (4096, tl, C4K), (4097, tl, STD), (8192, tl, STD)} <= seen
    assert {(4095, 14, STD), (4096, 14, STD), (4097, 14, STD), (8192, 14, STD)} <= seen
    low = _unit(next(c for c in CASES if c.name == "top4095/tl13"))
    assert (low.norm[-3:] == -1).all() and _inst(low) == C4K                 # -1 counts at the top of a compact unit's alphabet
    assert all(M.nbig(_unit(c).norm, c.flavour) >= 1 for c in CASES if c.flavour != 108)   # a symbol of more than sixteen slots, everywhere
    assert _inst(_unit(next(c for c in CASES if c.flavour == 108))) == STD
    assert _inst(_unit(next(c for c in CASES if c.flavour == 4))) == C4K


def _encode_check(mic, mico, sess, cases, d_sym, sym_off, counts):
    d_blobs, offs, st, _ = D.fse_encode_batch(mic, sess, d_sym.data_ptr(), sym_off[:-1], counts, [c.flavour for c in cases], [c.req_tl for c in cases])
    host = D.d2h(d_blobs, int(offs[-1])).copy()
    for i, c in enumerate(cases):
        u, want = _unit(c), _blob(mico, c)
        assert st[i] == 0, (c.name, "status", int(st[i]))
        got = host[int(offs[i]):int(offs[i + 1])].tobytes()
        if got != want:
            k = next((k for k in range(min(len(got), len(want))) if got[k] != want[k]), min(len(got), len(want)))
            raise AssertionError((c.name, "first differing blob byte", k, len(got), len(want)))
        r = D.route(mic, sess, i)
        assert r == u.enc_route(), (c.name, "route", sorted(M.names(r)), r >> 16, "model", sorted(M.names(u.enc_route())), u.enc_route() >> 16)
        assert _tab_inst(mic, sess, i) == _inst(u), (c.name, "encode instance", _tab_inst(mic, sess, i), _inst(u))
    return host.tobytes()


def _decode_check(mic, mico, sess, cases, torch):
    blobs = [_blob(mico, c) for c in cases]
    begins, pos = [], 0
    for i, b in enumerate(blobs):
        pos = (pos + 15) // 16 * 16 + (5 * i) % 16
        begins.append(pos)
        pos += len(b)
    ends = [a + len(b) for a, b in zip(begins, blobs)]
    host = np.full(pos + 64, 0xA5, np.uint8)
    for a, b in zip(begins, blobs):
        host[a:a + len(b)] = np.frombuffer(b, np.uint8)
    d_blobs = torch.from_numpy(host).cuda()
    caps = [_symbols(c).size for c in cases]
    st = D.fse_decode_batch(mic, sess, d_blobs.data_ptr(), begins, ends, [n + 64 for n in caps])
    back = []
    for i, c in enumerate(cases):
        u = _unit(c)
        assert st[i] == 0, (c.name, "decode status", int(st[i]))
        tok = D.tokens(mic, sess, i, caps[i])
        bad = np.flatnonzero(tok != _symbols(c))
        assert not bad.size, (c.name, "first differing symbol", int(bad[0]))
        r = D.route(mic, sess, i)
        assert r == u.dec_route(len(blobs[i])), (c.name, "route", sorted(M.names(r)), r >> 16, "model", sorted(M.names(u.dec_route(len(blobs[i])))))
        assert _tab_inst(mic, sess, i) == _inst(u), (c.name, "decode instance", _tab_inst(mic, sess, i), _inst(u))
        back.append(tok.tobytes())
    return back


def _run_twice(mic, mico, cases):
    torch = pytest.importorskip("torch")
    syms = [_symbols(c) for c in cases]
    counts = [s.size for s in syms]
    sym_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    d_sym = torch.from_numpy(np.concatenate(syms).view(np.int16)).cuda()
    sess = mic.Session(len(cases), 4096)
    try:
        enc = [_encode_check(mic, mico, sess, cases, d_sym, sym_off, counts) for _ in range(2)]
        assert enc[0] == enc[1]
        dec = [_decode_check(mic, mico, sess, cases, torch) for _ in range(2)]
        assert dec[0] == dec[1]
    finally:
        sess.close()


def test_a_batch_that_mixes_the_classes(mic, mico, gpu_ready):
    order = [CASES[(7 * i) % len(CASES)] for i in range(len(CASES))]        # (15 cases, 7 coprime: every case once, the classes interleaved)
    assert len({c.name for c in order}) == len(CASES)
    _run_twice(mic, mico, order)


def _tiny_kinds():
    kinds = []
    for k in range(8):                                                      # eight alphabets of 50 .. 225 symbols, 4096 tokens each
        top = 49 + 25 * k
        h = np.zeros(top + 1, np.int64)
        body = np.exp(-np.arange(top + 1) / (6.0 + k))                       # (steep: the first symbols take more than sixteen slots)
        h[:] = np.maximum(np.round(body / body.sum() * (3900 - top)).astype(np.int64), 1)
        h[0] += 4096 - h.sum()
        assert h.sum() == 4096 and h.min() >= 1
        c = Case(f"tiny{k}", h, 2, 0, None)
        u = _unit(c)
        assert u.rc == 0 and _inst(u) == C4K and M.nbig(u.norm, 2) >= 1, (c.name, u.rc, u.tl)
        kinds.append(c)
    return kinds


def test_six_hundred_tiny_units_are_more_than_one_resident_round(mic, mico, gpu_ready):
    kinds = _tiny_kinds()
    _run_twice(mic, mico, [kinds[(3 * i) % 8] for i in range(600)])


def test_small_frame_strips_take_the_compact_instance(mic, mico, synth, gpu_ready):
    """two 12-bit strips through the ordinary Session calls: their tokens stay below 4096, the oracle's bytes, the pixels back"""
    torch = pytest.importorskip("torch")
    W, H = 322, 64
    imgs = [synth.xr_like(cols=W, rows=H, depth=12, seed=3 + i) for i in range(2)]
    host = np.stack(imgs)
    d_px = torch.from_numpy(host.view(np.int16)).cuda()
    d_out = torch.zeros_like(d_px)
    units = [(i * W * H, W, H, 4095, 2) for i in range(2)]
    sess = mic.Session(len(units), W * H)
    try:
        cu = mic.Session.make_units(units)
        for again in range(2):
            sess.encode_enqueue(d_px.data_ptr(), cu)
            d_blobs, offs, st, ns = sess.encode_finish()
            assert (np.asarray(st) == 0).all()
            got = D.d2h(d_blobs, int(offs[-1]))
            for i, img in enumerate(imgs):
                rc, want = mico.compress_single_frame(img, 4095, 2)
                assert rc == 0 and got[int(offs[i]):int(offs[i + 1])].tobytes() == want, ("strip", i)
                assert D.words(mic, sess, i)[3] <= C4K_SYMS and _tab_inst(mic, sess, i) == C4K, ("strip", i, D.words(mic, sess, i)[:8])
            sess.decode_enqueue(d_blobs, offs, cu, d_out.data_ptr())
            dst = sess.decode_finish()
            assert (np.asarray(dst) == 0).all() and torch.equal(d_out, d_px)
            assert all(_tab_inst(mic, sess, i) == C4K for i in range(2))
    finally:
        sess.close()


def test_a_session_that_has_not_seen_the_compact_class_lately_still_decodes_it(mic, mico, synth, gpu_ready):
    """the compact decode instance is launched when the session's class memory (or no memory) allows a tableLog <= 13 stream; behind
    a batch of tableLog-14 streams it is not, and the standard instance, the catch-all, builds the strip's table: the same pixels,
    tb_inst says STD once, and the compact instance is back on the next call"""
    torch = pytest.importorskip("torch")
    import decode_class_streams as DC
    deep = DC.class_batch(mico, 14, 2, 0)[:2]
    assert all(s.table_log == 14 for s in deep)
    W, H = 322, 64
    img = synth.xr_like(cols=W, rows=H, depth=12, seed=5)
    rc, blob = mico.compress_single_frame(img, 4095, 2)
    assert rc == 0

    def decode(sess, blobs, dims, maxvs):
        offs = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
        host = np.zeros(int(offs[-1]) + 64, np.uint8)
        host[:int(offs[-1])] = np.frombuffer(b"".join(blobs), np.uint8)
        d_blobs = torch.from_numpy(host).cuda()
        px = np.concatenate([[0], np.cumsum([w * h for w, h in dims])])
        d_out = torch.zeros(int(px[-1]), dtype=torch.int16, device="cuda")
        tab = mic.Session.make_units([(int(px[i]), dims[i][0], dims[i][1], maxvs[i], 2) for i in range(len(blobs))])
        sess.decode_enqueue(d_blobs.data_ptr(), offs, tab, d_out.data_ptr())
        st = sess.decode_finish()
        out = d_out.cpu().numpy().view(np.uint16)
        return list(st), [out[px[i]:px[i + 1]].reshape(dims[i][1], dims[i][0]) for i in range(len(blobs))]

    sess = mic.Session(2, max([W * H] + [s.img.size for s in deep]))
    try:
        st, imgs = decode(sess, [s.blob for s in deep], [s.dims for s in deep], [s.maxv for s in deep])
        assert st == [0, 0] and all(np.array_equal(a, s.img) for a, s in zip(imgs, deep))
        assert [_tab_inst(mic, sess, i) for i in range(2)] == [STD, STD]
        for want in (STD, C4K, C4K):
            st, imgs = decode(sess, [blob], [(W, H)], [4095])
            w = D.words(mic, sess, 0)
            assert st == [0] and np.array_equal(imgs[0], img) and w[2] <= C4K_TL and w[3] <= C4K_SYMS, (want, st, w[:8])
            assert _tab_inst(mic, sess, 0) == want, (want, _tab_inst(mic, sess, 0))
    finally:
        sess.close()
