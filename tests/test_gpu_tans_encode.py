"""The tANS encode stage (csrc/mic_encode.hip: k_enc_tans_wg in its seven instances, te_encode, te_pack, k_enc_tans_pack,
k_enc_tans_serial) at the seams of its partition, its classes, its fix-up loop, its pack pass and its fallback chain, and a record of
WHICH kernel coded each unit.

The units come from tests/tans_encode_streams.py, one batch of bare token streams per group; tests/test_tans_encode_cpu.py shows on the
CPU that the oracle alone carries each case, that the model of tests/tans_encode_model.py writes the oracle's bytes, and that each case
reaches the seam it is named for.  A batch runs side by side in one launch chain through the debug door
mic_hip_debug_fse_encode_enqueue (the chain group through mic_hip_debug_fse_encode_chain_enqueue, which lets the fallback chain and
the two-state instance's hand-over run), on a fresh session and once more on the same one.

Every unit must agree with the oracle on its status and on its packed bytes, byte for byte, with the chain on the flavour it ends on,
and with the model on MicUnit.enc_kernel -- k_enc_tans_serial is always launched, takes whatever the class kernels leave and writes
the same bytes, so a gate that stopped matching would otherwise pass everything -- on MicUnit.enc_rounds, the fix-up rounds of the
attempt that decided the unit, and on whether the two-state instance handed the unit over.  The packed buffer must be the oracle's
blobs end to end, and the bytes behind the last unit (a tiny one in the pack group, whose last word is shared) must be left alone: the
first run leaves sentinels there and the second, which packs to the same place, must not have touched them.  The door launches every class, so no
unit of these batches may come from the serial kernel."""
import ctypes as C

import numpy as np
import pytest

import table_doors as D
import tans_encode_model as E
import tans_encode_streams as S

pytestmark = pytest.mark.gpu


SENTINEL, BEHIND = 0xA5, 64                                                 # bytes behind the last unit of a batch that no pack kernel may touch


def _check(mic, mico, sess, cases, host, offs, st, used, again):
    want_buf = []
    for i, c in enumerate(cases):
        name = (c.name, "again" if again else "fresh")
        rc, lanes, blob = S.reference(mico, c)
        u, r = S.unit(c), S.model(c)
        kernel, rounds, handed = D.enc_kernel(mic, sess, i)
        assert st[i] == rc, (name, "status", int(st[i]), "oracle", rc)
        got = host[int(offs[i]):int(offs[i + 1])].tobytes()
        if got != blob:
            k = next((k for k in range(min(len(got), len(blob))) if got[k] != blob[k]), min(len(got), len(blob)))
            raise AssertionError((name, "first differing blob byte", k, len(got), len(blob), got[k:k + 8].hex(), blob[k:k + 8].hex()))
        want_buf.append(blob)
        if rc == 0:
            assert used[i] == lanes, (name, "nstates_used", int(used[i]), "chain ends on", lanes)
        if r is None:                                                       # refused in front of the tANS stage: nobody's
            assert (kernel, rounds, handed) == (0, 0, False), (name, kernel, rounds, handed)
            continue
        assert kernel != E.SERIAL, (name, "coded by k_enc_tans_serial; the model names", E.KERNELS[r.kernel])
        assert kernel == r.kernel, (name, "enc_kernel", E.KERNELS.get(kernel, kernel), "model", E.KERNELS[r.kernel])
        assert handed == r.handed, (name, "handed over", handed, "model", r.handed, r.attempts)
        assert rounds == r.rounds, (name, "enc_rounds", rounds, "model", r.rounds)
    # the bytes between and around the units are the neighbours' own: the packed buffer is the oracle's blobs end to end
    assert host[:int(offs[-1])].tobytes() == b"".join(want_buf), "packed buffer"
    if again:                                                               # ... and behind the last unit nothing was stored (the first run left sentinels there)
        tail = host[int(offs[-1]):int(offs[-1]) + BEHIND]
        assert tail.size == BEHIND and (tail == SENTINEL).all(), ("bytes behind the last unit", tail.tobytes().hex())


@pytest.mark.parametrize("group", S.GROUPS)
def test_units_are_coded_by_the_kernel_the_model_names_and_carry_the_oracles_bytes(mic, mico, gpu_ready, group):
    torch = pytest.importorskip("torch")
    cases = S.group(group)
    chain = cases[0].chain
    assert all(c.chain == chain for c in cases)
    syms = [S.symbols(c) for c in cases]
    sym_off = np.concatenate([[0], np.cumsum([s.size for s in syms])]).astype(np.uint64)
    d_sym = torch.from_numpy(np.concatenate(syms).view(np.int16)).cuda()
    sess = mic.Session(len(cases), 4096)
    try:
        for again in range(2):
            d_blobs, offs, st, used = D.fse_encode_batch(mic, sess, d_sym.data_ptr(), sym_off[:-1], [s.size for s in syms],
                                                         [c.flavour for c in cases], [c.req_tl for c in cases], chain=chain)
            total = int(offs[-1])
            if again:
                assert (d_blobs, total) == first, "the second run packs into the same buffer, to the same length"
            _check(mic, mico, sess, cases, D.d2h(d_blobs, total + (BEHIND if again else 0)), offs, st, used, again)
            if not again:                                                   # (the packed buffer is at least 64 KiB longer than the batch: session_encode_finish)
                first = (d_blobs, total)
                assert C.cdll.LoadLibrary("libamdhip64.so").hipMemset(C.c_void_p(d_blobs + total), SENTINEL, C.c_size_t(BEHIND)) == 0
    finally:
        sess.close()
