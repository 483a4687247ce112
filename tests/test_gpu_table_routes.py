"""The FSE table kernels (k_enc_tables_wg, k_dec_parse<BIG>, k_dec_tables_wg in csrc/mic_tables.hip; tp_build in
csrc/mic_tables_par.h; the window reader of mic_read_ncount) at their normaliser, header, scratch, spread and parse seams, and a record
of WHICH fork handled each unit.

The units come from tests/table_streams.py, one batch of bare FSE units per group; tests/test_table_routes_cpu.py shows on the CPU
that the oracle alone carries each case and that each reaches the seam it is named for.  A batch runs side by side in one launch chain
through the debug doors mic_hip_debug_fse_encode_enqueue / mic_hip_debug_fse_decode_enqueue (thin bindings in tests/table_doors.py:
they are no part of the package), on a fresh session and once more on the same one.

After the encode every unit must agree with the oracle on its status, its blob byte for byte and its facts, with the model of
tests/table_routes.py on MicUnit.tb_route -- a parallel normaliser or writer that always declined would otherwise pass everything,
because the serial fallback writes the same bytes -- and on its encode tables entry by entry.  Of the table slabs, state_tab, tt_nb and
tt_find are intact behind the tANS kernels of the same chain (they only read them) and are compared; norm is not compared on the
encode side (the LDS class never writes the slab) and neither are hist, cumul and tab_sym (scratch of the HBM class, hist re-zeroed
behind the chain).  rANS units have no state table.

Then the oracle's blobs are decoded at every byte lead 0 .. 15 (the 16-byte `head` of the staging copy takes every value for every
unit): symbols, parsed facts, parse route and the whole decode table -- tt_nb[0:size], tab_sym[0:size], also the entries the stream
never visits -- and norm[0:symbol_len], all intact behind the decode chain.

Where the reference has no behaviour (normalizeCount2 with every slot given away divides by zero or spins) the expected status is
the oracle's, -8."""
import numpy as np
import pytest

import table_doors as D
import table_routes as M
import table_streams as S

pytestmark = pytest.mark.gpu

def _same_route(name, got, want):
    assert got == want, (name, "route", sorted(M.names(got)), got >> 16, "model", sorted(M.names(want)), want >> 16)


def _same_entries(name, what, got, want, where=None, norm=None):
    """entry by entry; `where` limits the comparison (symbols that occur)"""
    idx = np.arange(want.size) if where is None else np.flatnonzero(where)
    bad = idx[got[idx] != want[idx]]
    if bad.size:
        k = int(bad[0])
        raise AssertionError((name, what, "first differing entry", k, "got", int(got[k]), "want", int(want[k]),
                              "count of that symbol" if norm is not None else "", int(norm[k]) if norm is not None else ""))


def _same_state_tab(name, u, got, want):
    bad = np.flatnonzero(got != want)
    if bad.size:
        k = int(bad[0])
        slots = M._slots(u.norm)
        sym = int(np.searchsorted(np.cumsum(slots), k, side="right"))
        raise AssertionError((name, "state_tab: first differing entry", k, "symbol", sym, "slot", k - int(np.cumsum(slots)[sym] - slots[sym]),
                              "got", int(got[k]), "want", int(want[k])))


_TABLES = {}


def _model_tables(c, u):
    key = (c.name, "tables")
    if key not in _TABLES:
        if c.flavour == 108:
            _TABLES[key] = (None,) + M.rans_ctable(u.norm, u.tl) + M.rans_dtable(u.norm, u.tl)
        else:
            st, nb, find, _ = M.ctable(u.norm, u.tl)
            _TABLES[key] = (st, nb, find) + M.dtable(u.norm, u.tl)
    return _TABLES[key]


def _check_encoded(mic, mico, sess, cases, host, offs, st):
    for i, c in enumerate(cases):
        u = S.unit(c)
        rc, facts, blob = S.reference(mico, c)
        w = D.words(mic, sess, i)
        assert st[i] == rc == D.i32(w[11]), (c.name, "status", int(st[i]), rc, D.i32(w[11]))
        got = host[int(offs[i]):int(offs[i + 1])].tobytes()
        if rc:
            assert got == b"", (c.name, len(got))
            continue
        head, want_head = got[u.prefix:u.prefix + u.hdr_len], blob[u.prefix:u.prefix + u.hdr_len]
        if head != want_head:
            k = next(k for k in range(min(len(head), len(want_head))) if head[k] != want_head[k]) if len(head) == len(want_head) else min(len(head), len(want_head))
            raise AssertionError((c.name, "first differing header byte", k, head[k:k + 4].hex(), want_head[k:k + 4].hex()))
        if got != blob:
            k = next((k for k in range(min(len(got), len(blob))) if got[k] != blob[k]), min(len(got), len(blob)))
            raise AssertionError((c.name, "first differing blob byte", k, len(got), len(blob)))
        # table_log, symbol_len, max_count, hdr_len; the ENCODER's zero-bits flag (a count above half the table, 0 for rANS)
        assert (w[2], w[3], w[4], w[5] + u.prefix, w[6]) == (facts["table_log"], facts["symbol_len"], facts["max_count"], facts["hdr_len"], u.enc_zero_bits), (c.name, w[:8])
        _same_route(c.name, D.route(mic, sess, i), u.enc_route())
        state_tab, tt_nb, tt_find, _, _ = _model_tables(c, u)
        occurs = u.norm != 0
        _same_entries(c.name, "tt_nb", D.table(mic, sess, i, D.TT_NB, u.symbol_len), tt_nb, occurs, u.norm)
        _same_entries(c.name, "tt_find", D.table(mic, sess, i, D.TT_FIND, u.symbol_len), tt_find, occurs, u.norm)
        if state_tab is not None:
            _same_state_tab(c.name, u, D.table(mic, sess, i, D.STATE_TAB, 1 << u.tl), state_tab)


@pytest.mark.parametrize("group", S.GROUPS)
def test_units_take_the_route_the_model_names_and_write_the_oracles_bytes(mic, mico, gpu_ready, group):
    torch = pytest.importorskip("torch")
    cases = S.group(group)
    syms = [S.symbols(c) for c in cases]
    sym_off = np.concatenate([[0], np.cumsum([s.size for s in syms])]).astype(np.uint64)
    d_sym = torch.from_numpy(np.concatenate(syms).view(np.int16)).cuda()
    sess = mic.Session(len(cases), 4096)
    try:
        for again in range(2):
            d_blobs, offs, st, _ = D.fse_encode_batch(mic, sess, d_sym.data_ptr(), sym_off[:-1], [s.size for s in syms],
                                                    [c.flavour for c in cases], [c.req_tl for c in cases])
            _check_encoded(mic, mico, sess, cases, D.d2h(d_blobs, int(offs[-1])), offs, st)
    finally:
        sess.close()


@pytest.mark.parametrize("group", S.GROUPS)
def test_the_oracles_blobs_parse_on_the_route_the_model_names_at_every_lead(mic, mico, gpu_ready, group):
    torch = pytest.importorskip("torch")
    cases = [c for c in S.group(group) if S.reference(mico, c)[0] == 0]
    blobs = [S.reference(mico, c)[2] for c in cases]
    caps = [S.symbols(c).size for c in cases]
    sess = mic.Session(len(cases), 4096)
    heads = [set() for _ in cases]
    try:
        for lead in range(16):
            begins, pos = [], 0
            for i, b in enumerate(blobs):
                pos = (pos + 15) // 16 * 16 + (lead + 3 * i) % 16
                begins.append(pos)
                pos += len(b)
            ends = [a + len(b) for a, b in zip(begins, blobs)]
            host = np.full(pos + 64, 0xA5, np.uint8)
            for a, b in zip(begins, blobs):
                host[a:a + len(b)] = np.frombuffer(b, np.uint8)
            d_blobs = torch.from_numpy(host).cuda()
            assert d_blobs.data_ptr() % 16 == 0
            st = D.fse_decode_batch(mic, sess, d_blobs.data_ptr(), begins, ends, [n + 64 for n in caps])
            for i, c in enumerate(cases):
                u = S.unit(c)
                _, facts, blob = S.reference(mico, c)
                name = (c.name, "lead", begins[i] % 16)
                heads[i].add(begins[i] % 16)
                w = D.words(mic, sess, i)
                assert st[i] == 0 == D.i32(w[11]), (name, "status", int(st[i]))
                # table_log, symbol_len, zero_bits, flavour, count, offset of the bitstream
                assert (w[2], w[3], w[6], w[7], w[8] if c.flavour != 1 else 0, w[9]) == \
                       (u.tl, u.symbol_len, facts["zero_bits"], c.flavour, caps[i] if c.flavour != 1 else 0, facts["hdr_len"]), (name, w[:12])
                _same_route(name, D.route(mic, sess, i), u.dec_route(len(blob)))
                _same_entries(name, "norm", D.table(mic, sess, i, D.NORM, u.symbol_len), u.norm.astype(np.int32))
                tab_sym, dt = _model_tables(c, u)[3:]
                _same_entries(name, "tab_sym", D.table(mic, sess, i, D.TAB_SYM, 1 << u.tl), tab_sym)
                _same_entries(name, "tt_nb", D.table(mic, sess, i, D.TT_NB, 1 << u.tl), dt)
                assert w[0] == caps[i], (name, "symbols", w[0], caps[i])
                tok = D.tokens(mic, sess, i, caps[i])
                want = S.symbols(c)
                bad = np.flatnonzero(tok != want)
                assert not bad.size, (name, "first differing symbol", int(bad[0]), int(tok[bad[0]]), int(want[bad[0]]))
        assert all(h == set(range(16)) for h in heads)
    finally:
        sess.close()
