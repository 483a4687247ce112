"""Thin ctypes bindings of the table stage's debug doors and probes (csrc/mic_api.hip; none of them is in the public header or in
the package): many bare FSE units in one launch chain of a caller's Session, the route record, the table slabs and the tokens of a
unit after a *_finish; and of the tANS encode stage's (the same encode door with the fallback chain, the record of which kernel coded
a unit).  They use the Session's handle and its unit count as Session.encode_finish / decode_finish do; the first
call checks that both are still there under those names.  Used by tests/test_gpu_table_routes.py and
tests/test_gpu_tans_encode.py."""
import ctypes as C

import numpy as np

STATE_TAB, TT_NB, TT_FIND, TAB_SYM, NORM = range(5)
_DT = {STATE_TAB: np.uint32, TT_NB: np.uint32, TT_FIND: np.int32, TAB_SYM: np.uint16, NORM: np.int32}


def _lib(mic):
    L = mic.lib()
    L.mic_hip_debug_fse_encode_enqueue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.mic_hip_debug_fse_encode_chain_enqueue.argtypes = L.mic_hip_debug_fse_encode_enqueue.argtypes
    L.mic_hip_debug_enc_kernel.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.mic_hip_debug_fse_decode_enqueue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.mic_hip_debug_tab_route.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.mic_hip_debug_fetch_table.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    L.mic_hip_debug_fetch_tok.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    return L


def d2h(d_ptr, nbytes):
    host = np.empty(max(nbytes, 1), np.uint8)
    if nbytes:
        assert C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(d_ptr), C.c_size_t(nbytes), 2) == 0
    return host[:nbytes]


def _session(sess):
    assert hasattr(sess, "_h") and hasattr(sess, "_n") and hasattr(sess, "encode_finish") and hasattr(sess, "decode_finish"), "Session's handle moved: rebind tests/table_doors.py"
    return sess._h


def fse_encode_batch(mic, sess, d_symbols, sym_off, counts, flavours, req_tl, chain=False):
    """N bare FSE units in one encode chain of `sess` -> what Session.encode_finish returns; chain: with the fallback chain
    N -> N / 2 -> ... -> 1 behind the table stage (mic_hip_debug_fse_encode_chain_enqueue)"""
    a = [np.ascontiguousarray(sym_off, np.uint64), np.ascontiguousarray(counts, np.uint32),
         np.ascontiguousarray(flavours, np.int32), np.ascontiguousarray(req_tl, np.int32)]
    door = _lib(mic).mic_hip_debug_fse_encode_chain_enqueue if chain else _lib(mic).mic_hip_debug_fse_encode_enqueue
    rc = door(_session(sess), d_symbols, *[x.ctypes.data for x in a], len(a[1]))
    assert rc == 0, rc
    sess._n = len(a[1])
    return sess.encode_finish()


def fse_decode_batch(mic, sess, d_blobs, begins, ends, caps):
    """N FSE streams at d_blobs + [begins[i], ends[i]) in one decode chain of `sess` -> status per unit"""
    a = [np.ascontiguousarray(begins, np.uint64), np.ascontiguousarray(ends, np.uint64), np.ascontiguousarray(caps, np.uint32)]
    rc = _lib(mic).mic_hip_debug_fse_decode_enqueue(_session(sess), d_blobs, *[x.ctypes.data for x in a], len(a[2]))
    assert rc == 0, rc
    sess._n = len(a[2])
    return sess.decode_finish()


def i32(v):
    return v - (1 << 32) if v & 0x80000000 else v


def words(mic, sess, i):
    buf = (C.c_uint32 * 32)()
    assert mic.lib().mic_hip_debug_unit(_session(sess), i, buf) == 0
    return [int(v) for v in buf]


def route(mic, sess, i):
    r = C.c_uint32()
    assert _lib(mic).mic_hip_debug_tab_route(_session(sess), i, C.byref(r)) == 0
    return int(r.value)


def enc_kernel(mic, sess, i):
    """(MicUnit.enc_kernel without its flag, MicUnit.enc_rounds, handed over) of unit i after an encode's *_finish"""
    out = (C.c_uint32 * 3)()
    assert _lib(mic).mic_hip_debug_enc_kernel(_session(sess), i, out) == 0
    return int(out[0]), int(out[1]), bool(out[2])


def table(mic, sess, i, which, entries):
    out = np.zeros(max(entries, 1), _DT[which])
    assert _lib(mic).mic_hip_debug_fetch_table(_session(sess), i, which, out.ctypes.data, entries * out.itemsize) == 0
    return out[:entries]


def tokens(mic, sess, i, n):
    tok = np.zeros(max(n, 1), np.uint16)
    assert _lib(mic).mic_hip_debug_fetch_tok(_session(sess), i, tok.ctypes.data, n) == 0
    return tok[:n]
