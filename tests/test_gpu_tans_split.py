"""The two-part instance of the two-state tANS chain (k_dec_tans_ls_parts<2>, csrc/mic_decode_ls.hip) at its seams, on small units.

The units are thin strips of the headline's frame (2577 columns, 24 .. 40 rows of 12-bit xr_like at the published noise: 60 - 100 k
tokens, about 9.6 bits each), coded by the oracle; the session's split gate and overlap are lowered through the debug setter so that
such units are split.  What the kernel must make of each unit -- split or handed back, and where the halves join -- is worked out on
the CPU by tests/tans_split_model.py; the library is asked for its record (MicUnit.split through mic_hip_debug_split) and for the
pixels, which must be the source's bit for bit.

The shapes a case is there for are asserted on the CPU side, in front of the GPU run."""
import ctypes as C
import functools

import numpy as np
import pytest

import decode_class_streams as D
import tans_split_model as M

pytestmark = pytest.mark.gpu

W_TEST = 4096                                      # overlap of the small units (the default, 32768, is half of such a unit)
MIN_TEST = 4096
TILE = 1536                                        # k_dec_translate's tile


class Unit:
    def __init__(self, mico, img):
        self.img, self.maxv = np.ascontiguousarray(img), 4095
        tok = mico.delta_rle_compress(self.img, self.maxv)
        self.model = M.Stream(mico, tok)
        rc, self.blob = mico.compress_single_frame(self.img, self.maxv, 2)
        assert rc == 0 and self.blob == self.model.blob
        self.ntok, self.hdr_len = self.model.count, self.model.hdr_len
        self.expected = {}

    @property
    def dims(self):
        return self.img.shape[1], self.img.shape[0]


def _strip(synth, seed, rows, noise=None):
    noise = synth.XR_NOISE_PUBLISHED_RATIO if noise is None else noise
    return synth.xr_like(cols=2577, rows=256, depth=12, seed=seed, noise=noise)[64:64 + rows]   # (a strip-high frame: away from its border rows)


def _with_tokens(mico, img, residue, mod=TILE):
    """`img` with a flat start that leaves a token count of `residue` modulo `mod` (a flat pixel more is about a token less)"""
    n0 = mico.delta_rle_compress(np.ascontiguousarray(img), 4095).size
    target = n0 - 8 - ((n0 - 8 - residue) % mod)
    k, tried = n0 - target, {}
    for _ in range(12):
        k = min(max(k, 3), img.shape[1] - 1)
        if k in tried:
            break
        tried[k] = mico.delta_rle_compress(D.with_flat_start(img, k), 4095).size
        if tried[k] == target:
            return D.with_flat_start(img, k)
        k += tried[k] - target
    for k in range(3, img.shape[1] - 1):
        if mico.delta_rle_compress(D.with_flat_start(img, k), 4095).size == target:
            return D.with_flat_start(img, k)
    raise AssertionError(f"no strip of {target} tokens")


@functools.lru_cache(maxsize=None)
def _units(mico, synth):
    """thirteen split candidates -- a full group, a full wave and one stream beside its clones -- of differing lengths; the first
    three end on k_dec_translate's tile edge, one token behind it and one in front of it (so also on the chunk's and the double
    chunk's), then a strip under the rate gate and one under the length gate"""
    u = [Unit(mico, _with_tokens(mico, _strip(synth, 20 + r, 24 + 2 * r), res)) for r, res in enumerate((0, 1, TILE - 1))]
    u += [Unit(mico, _strip(synth, seed, rows)) for seed, rows in ((5, 24), (7, 32), (9, 40), (11, 24), (13, 28), (14, 25), (15, 27),
                                                                  (16, 31), (17, 36), (18, 24))]
    quiet = Unit(mico, _strip(synth, 3, 40, noise=3.0))
    short = Unit(mico, _strip(synth, 4, 1, noise=18.0))
    return u, quiet, short


def _lib(mic):
    L = mic.lib()
    L.mic_hip_debug_split.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.mic_hip_debug_split_config.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    return L


def _configure(mic, sess, min_tokens=MIN_TEST, overlap=W_TEST):
    assert _lib(mic).mic_hip_debug_split_config(sess._h, min_tokens, overlap, 0) == 0


def _decode(mic, torch, sess, units, blobs=None, lead=0):
    """one decode of the units' blobs laid end to end from byte `lead` on -> (status, dec_kernel, split record, images, bitstream
    address & 3) per unit"""
    blobs = [u.blob for u in units] if blobs is None else blobs
    offs = np.zeros(len(units) + 1, np.uint64)
    offs[0] = lead
    offs[1:] = lead + np.cumsum([len(b) for b in blobs])
    host = np.zeros(int(offs[-1]) + 64, np.uint8)
    host[lead:int(offs[-1])] = np.frombuffer(b"".join(blobs), np.uint8)
    d_blobs = torch.from_numpy(host).cuda()
    px = np.concatenate([[0], np.cumsum([u.img.size for u in units])]).astype(np.int64)
    tab = mic.Session.make_units([(int(px[i]), u.dims[0], u.dims[1], u.maxv, 2) for i, u in enumerate(units)])
    d_out = torch.zeros(int(px[-1]), dtype=torch.int16, device="cuda")
    sess.decode_enqueue(d_blobs.data_ptr(), offs, tab, d_out.data_ptr())
    st = sess.decode_finish()
    rec, split = [], []
    for i in range(len(units)):
        buf = (C.c_uint32 * 32)()
        assert mic.lib().mic_hip_debug_unit(sess._h, i, buf) == 0
        rec.append(int(buf[15]))
        out = (C.c_uint32 * 3)()
        assert _lib(mic).mic_hip_debug_split(sess._h, i, out) == 0
        split.append(tuple(int(v) for v in out))
    out = d_out.cpu().numpy().view(np.uint16)
    imgs = [out[px[i]:px[i + 1]].reshape(u.img.shape) for i, u in enumerate(units)]
    align = [(d_blobs.data_ptr() + int(offs[i]) + u.hdr_len) & 3 for i, u in enumerate(units)]
    return st, rec, split, imgs, align


def _expect(u, overlap, min_tokens=MIN_TEST):
    """what MicUnit.split must hold of the unit (worked out once per unit and overlap)"""
    if not u.model.gate(min_tokens=min_tokens):
        return (M.NOT_TRIED, 0, 0)
    if overlap not in u.expected:
        o, i, j = u.model.split(overlap)
        u.expected[overlap] = (o, i, j) if o in (M.DONE, M.NO_ROOM, M.BAD_COUNT) else (o, 0, j)
    return u.expected[overlap]


def _check(units, want, st, rec, split, imgs):
    for i, u in enumerate(units):
        assert st[i] == 0, (i, st[i])
        assert split[i] == want[i], (i, split[i], want[i], u.ntok)
        if u.model.table_log == 13 and not u.model.zero_bits:
            assert rec[i] == 1, (i, rec[i])                                 # class 0's record, split or not
        assert np.array_equal(imgs[i], u.img), (i, u.ntok, split[i])


def test_split_units_join_where_the_model_says(mic, mico, synth, gpu_ready):
    torch = pytest.importorskip("torch")
    cand, quiet, short = _units(mico, synth)
    want = [_expect(u, W_TEST) for u in cand]
    done = [w for w in want if w[0] == M.DONE]
    # the CPU side: the seams this batch is there for
    assert len(done) >= 9 and any(w[0] == M.NOT_MET for w in want), want     # (a unit whose halves do not meet inside 4096 symbols rides along)
    assert {(w[1] - w[2]) & 1 for w in done} == {0, 1}                        # part 1's lanes in step with the symbol parity, and role-swapped
    assert any(w[1] % 8 for w in done)                                        # the join inside a translate thread's eight tokens
    assert [u.ntok % TILE for u in cand[:3]] == [0, 1, TILE - 1]
    assert [u.ntok % 64 for u in cand[:3]] == [0, 1, 63] and [u.ntok % 128 for u in cand[:3]] == [0, 1, 127]
    assert len({u.ntok // 64 for u in cand}) >= 8                             # lengths differ by whole chunks
    assert quiet.ntok >= MIN_TEST and not quiet.model.gate(min_tokens=MIN_TEST) and short.ntok < MIN_TEST
    sess = mic.Session(len(cand) + 2, max(u.img.size for u in cand + [quiet]))
    try:
        _configure(mic, sess)
        seen, first = set(), None
        # 13 candidates: a last wave of one stream; 11, 12: of two and three (behind a full group); mixed: unsplit units in between
        for lead, units in ((0, cand), (0, cand), (1, cand[:11]), (2, cand[:12]), (3, cand[:5] + [quiet] + cand[5:8] + [short] + cand[8:])):
            w = [_expect(u, W_TEST) for u in units]
            st, rec, split, imgs, align = _decode(mic, torch, sess, units, lead=lead)
            _check(units, w, st, rec, split, imgs)
            seen |= {a for a, x in zip(align, w) if x[0] == M.DONE}
            if units is cand:                                                 # two consecutive decodes: the same records, the same pixels
                if first is None:
                    first = (list(st), rec, split, imgs)
                else:
                    assert (list(st), rec, split) == first[:3] and all(np.array_equal(a, b) for a, b in zip(imgs, first[3]))
        assert seen == {0, 1, 2, 3}                                           # a split unit's bitstream at each of the four byte offsets
    finally:
        sess.close()


# (seed, rows, overlap) whose halves join within eight tokens of a tile edge of k_dec_translate, from a search on the CPU model
EDGE_CASES = [(9, 40, 7296), (36, 24, 4480), (32, 24, 7424)]   # i_sync mod 1536 = 1529, 1535, 3: the join in a tile's last and first eight tokens


@pytest.mark.parametrize("seed,rows,overlap", EDGE_CASES)
def test_a_join_next_to_a_translate_tile_edge(mic, mico, synth, gpu_ready, seed, rows, overlap):
    torch = pytest.importorskip("torch")
    u = Unit(mico, _strip(synth, seed, rows))
    want = _expect(u, overlap)
    assert want[0] == M.DONE and (want[1] % TILE >= TILE - 8 or want[1] % TILE < 8), want
    sess = mic.Session(1, u.img.size)
    try:
        _configure(mic, sess, overlap=overlap)
        st, rec, split, imgs, _ = _decode(mic, torch, sess, [u])
        _check([u], [want], st, rec, split, imgs)
    finally:
        sess.close()


def test_an_overlap_too_small_to_meet_in_hands_the_unit_back(mic, mico, synth, gpu_ready):
    torch = pytest.importorskip("torch")
    cand = _units(mico, synth)[0][3:8]
    want = [_expect(u, 64) for u in cand]
    assert sum(w[0] == M.NOT_MET for w in want) >= 4, want                    # (64 symbols: a wrong start is forgotten in about 1500)
    sess = mic.Session(len(cand), max(u.img.size for u in cand))
    try:
        _configure(mic, sess, overlap=64)
        for _ in range(2):
            st, rec, split, imgs, _ = _decode(mic, torch, sess, cand)
            _check(cand, want, st, rec, split, imgs)
    finally:
        sess.close()


def test_a_stream_shorter_than_the_overlap_beside_a_longer_one(mic, mico, synth, gpu_ready):
    """the per-stream chunk cap: the hand-over after W = 65536 symbols lies behind everything a 60 k-token strip has to decode, but
    inside its 100 k-token neighbour's chunks, so the wave's loop runs up to the hand-over all the same; the short unit is not met
    (its own cap, the model's rule) and comes back through the retry list, the long one is handed over and recorded as modelled"""
    torch = pytest.importorskip("torch")
    cand = _units(mico, synth)[0]
    W, units = 65536, [cand[3], cand[5]]                                      # 24 and 40 rows
    want = [_expect(u, W) for u in units]
    # the CPU side: Wc against each stream's own cap; both pass the gate onto the two-part list, where they are neighbours: units 0
    # and 1 of the batch are streams 0 and 1 of the first wave
    assert W // 64 >= units[0].ntok // 64 + 2 and W // 64 < units[1].ntok // 64 + 2, [u.ntok for u in units]
    assert all(M.route(u.model, min_tokens=MIN_TEST) == M.TWO_PARTS for u in units)
    assert want[0] == (M.NOT_MET, 0, W) and want[1][0] != M.NOT_TRIED and want[1][2] == W, want
    sess = mic.Session(len(units), max(u.img.size for u in units))
    try:
        _configure(mic, sess, overlap=W)
        st, rec, split, imgs, _ = _decode(mic, torch, sess, units)
        _check(units, want, st, rec, split, imgs)
    finally:
        sess.close()


def test_a_damaged_second_half_is_judged_as_without_the_split(mic, mico, synth, gpu_ready):
    """a stream cut in its second half, and one with a bit flipped in part 1's range, among whole neighbours: status and pixels
    are those of the same session's unsplit decode of the same bytes, and the oracle's status"""
    torch = pytest.importorskip("torch")
    cand = _units(mico, synth)[0][3:8]
    victim = 2
    u = cand[victim]
    cut = u.blob[:u.hdr_len] + u.blob[u.hdr_len + 300:]                       # the bytes read last are gone: the count runs past bit 0
    flip = bytearray(u.blob)
    flip[u.hdr_len + (len(u.blob) - u.hdr_len) // 5] ^= 0x08
    assert u.model.split_start(W_TEST) // 8 > (len(u.blob) - u.hdr_len) // 5 + 600    # (inside part 1's range, below the meeting point)
    sess = mic.Session(len(cand), max(x.img.size for x in cand))
    try:
        for bad in (cut, bytes(flip)):
            rc_o, _ = mico.decompress_single_frame(bad, *u.dims)
            blobs = [bad if i == victim else x.blob for i, x in enumerate(cand)]
            _configure(mic, sess, min_tokens=1 << 30)                         # nothing is split
            st0, rec0, split0, imgs0, _ = _decode(mic, torch, sess, cand, blobs=blobs)
            assert all(s[0] == M.NOT_TRIED for s in split0)
            _configure(mic, sess)
            st1, rec1, split1, imgs1, _ = _decode(mic, torch, sess, cand, blobs=blobs)
            assert split1[victim][0] != M.NOT_TRIED and sum(s[0] == M.DONE for s in split1) >= 3, split1
            assert list(st1) == list(st0) and st1[victim] == rc_o, (list(st0), list(st1), rc_o)
            for i, x in enumerate(cand):
                if st1[i] == 0:
                    assert np.array_equal(imgs1[i], imgs0[i]), i
                if i != victim:
                    assert st1[i] == 0 and np.array_equal(imgs1[i], x.img), i
    finally:
        sess.close()
