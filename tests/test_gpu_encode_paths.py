"""GPU tests of where the encoder's streams are written.  The two-state 512-thread tANS instance packs its units straight into the
session's packed buffer (k_enc_tans_pack) next to units that k_enc_pack copies there; a unit's first and last bytes share words with
its neighbours.  Every unit must equal the oracle's stream byte for byte: with its borders at every offset modulo 32, between units of
every other class, and both when the batch fits the packed buffer and when it does not (the first batch of a session packs again)."""
import ctypes as C

import numpy as np
import pytest

import gap_ref

pytestmark = pytest.mark.gpu


def _d2h(d_ptr, nbytes):
    host = np.empty(nbytes, np.uint8)
    assert C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(d_ptr), C.c_size_t(nbytes), 2) == 0
    return host


def _run(mic, sess, d_px, units):
    sess.encode_enqueue(d_px.data_ptr(), units)
    d_blobs, offs, st, _ = sess.encode_finish()
    return _d2h(d_blobs, int(offs[-1])), offs, st


def _check(host, offs, st, want):
    for k, (rc, blob) in enumerate(want):
        assert st[k] == rc, (k, st[k], rc)
        if rc == 0:
            assert host[int(offs[k]):int(offs[k + 1])].tobytes() == blob, k


def test_unit_borders_at_every_offset_mod_32(mic, mico, synth, gpu_ready):
    """Ragged two-state XR units chosen (from the oracle's sizes) so that the running offset takes every value modulo 32; the
    frame's first rows are incompressible, and those failed units sit between the others."""
    torch = pytest.importorskip("torch")
    W, H = 333, 1200
    img = synth.xr_like(cols=W, rows=H, depth=12, seed=31)
    pool, failed = [], []                                             # (y0, rows, oracle rc, oracle stream)
    y0 = 0
    for rows in [5, 6, 7, 9, 11, 13, 17, 19, 23] * 8:
        if y0 + rows > H:
            break
        rc, blob = mico.compress_single_frame(img[y0:y0 + rows], 4095, 2)
        (pool if rc == 0 else failed).append((y0, rows, rc, blob))
        y0 += rows
    assert failed and len(pool) > 48
    # greedy order: each next unit ends at a residue not yet seen
    order, seen, off = [], {0}, 0
    left = list(range(len(pool)))
    while left and len(seen) < 32:
        pick = next((i for i in left if (off + len(pool[i][3])) % 32 not in seen), left[0])
        order.append(pick); left.remove(pick); off += len(pool[pick][3])
        seen.add(off % 32)
    assert len(seen) == 32
    specs = [pool[i] for i in order + left]
    for k, f in enumerate(failed):
        specs.insert(1 + 4 * k, f)
    units = mic.Session.make_units([(y * W, W, r, 4095, 2) for (y, r, _, _) in specs])
    d_px = torch.from_numpy(img.view(np.int16).copy()).cuda()
    sess = mic.Session(len(specs), W * 23)
    try:
        for _ in range(2):                                            # the first call packs twice (no size hint yet), the second once
            host, offs, st = _run(mic, sess, d_px, units)
            assert {int(o) % 32 for o in offs} == set(range(32))
            _check(host, offs, st, [(rc, b) for (_, _, rc, b) in specs])
    finally:
        sess.close()


def test_two_state_units_between_every_other_class(mic, mico, synth, gpu_ready):
    """Two-state XR units alternate with 4- and 8-state units, a 16-bit CT frame (tableLog past 13), gap-removal units (XR and CT)
    and a unit that fails (five incompressible rows)."""
    torch = pytest.importorskip("torch")
    from conftest import GOLDEN
    import os
    ct = np.fromfile(os.path.join(GOLDEN, "CT_512_512_image.bin"), dtype="<u2").reshape(512, 512)
    bad = synth.xr_like(cols=333, rows=1200, depth=12, seed=31)[:5]
    others = [(None, 4095, 4), (None, 4095, 8), (ct, 65535, 2), (None, 4095, 2 | mic.MIC_HIP_GAP_REMOVAL),
              (ct, 65535, 2 | mic.MIC_HIP_GAP_REMOVAL), (bad, 4095, 2), (ct, 65535, 4)]
    frames, specs = [], []                                            # specs: (max value, nstates | flags)
    for k, (px, mv, ns) in enumerate(others):
        frames.append(synth.xr_like(cols=512, rows=512, depth=12, seed=100 + k)); specs.append((4095, 2))
        frames.append(px if px is not None else synth.xr_like(cols=512, rows=512, depth=12, seed=200 + k)); specs.append((mv, ns))
    frames.append(synth.xr_like(cols=512, rows=512, depth=12, seed=99)); specs.append((4095, 2))
    want = []
    for px, (mv, ns) in zip(frames, specs):
        if ns & mic.MIC_HIP_GAP_REMOVAL:
            rc, blob, _ = gap_ref.compress(mico, px, mv, ns & 0xFF)
        else:
            rc, blob = mico.compress_single_frame(px, mv, ns & 0xFF)
        want.append((rc, blob))
    assert sum(rc != 0 for rc, _ in want) == 1
    offs = np.cumsum([0] + [f.size for f in frames])
    units = mic.Session.make_units([(int(offs[i]), f.shape[1], f.shape[0], mv, ns) for i, (f, (mv, ns)) in enumerate(zip(frames, specs))])
    d_px = torch.from_numpy(np.concatenate([f.ravel() for f in frames]).astype(np.uint16).view(np.int16)).cuda()
    sess = mic.Session(len(frames), 512 * 512)
    try:
        for _ in range(2):
            host, offs_dev, st = _run(mic, sess, d_px, units)
            _check(host, offs_dev, st, want)
    finally:
        sess.close()


def test_bench_shaped_strips_match_the_oracle(mic, mico, synth, gpu_ready):
    """Full-width XR strips (2577 columns: a collimator run crosses every row end) as bench.py cuts them, in a batch that does not fit
    the first packed buffer and then in one that does."""
    torch = pytest.importorskip("torch")
    W, H, S = 2577, 512, 8
    imgs = [synth.xr_like(cols=W, rows=H, depth=12, seed=300 + i) for i in range(3)]
    rows = H // S
    units, want = [], []
    for i, img in enumerate(imgs):
        for s in range(S):
            units.append((i * W * H + s * rows * W, W, rows, 4095, 2))
            want.append(mico.compress_single_frame(img[s * rows:(s + 1) * rows], 4095, 2))
    d_px = torch.from_numpy(np.stack(imgs).view(np.int16).copy()).cuda()
    sess = mic.Session(len(units), W * rows)
    try:
        cu = mic.Session.make_units(units)
        for _ in range(2):
            host, offs, st = _run(mic, sess, d_px, cu)
            _check(host, offs, st, want)
    finally:
        sess.close()
