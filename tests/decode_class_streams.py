"""Frame streams for every decode class of csrc/mic_decode_ls.hip, made on the CPU (tests/test_gpu_decode_classes.py, and
tests/test_decode_classes_cpu.py for what can be checked without a device).

A frame stream is FSE(delta_rle_compress(image)) with nothing around it, so the oracle's FSECompressU16* with a requested tableLog
writes a legal frame blob of any flavour and any tableLog optimal_table_log (oracle/mic_oracle_core.c) allows: at most
highbit(tokens - 1) - 2.  Eight-bit images keep the alphabet under 256 symbols, so the token COUNT alone decides the largest tableLog
and the request picks it.  Token counts are exact: a frame's first k pixels of row 0 are made equal, which turns k literal tokens
into a run of two per 124, and k is solved for against the oracle's own tokeniser.

Nothing here knows what the library thinks of a stream: `dec_cls` restates mic_dec_cls (csrc/mic_launch.h) and the geometry table
restates LsGeom (csrc/mic_decode_ls.hip); the CPU test compares both with the sources by value."""
import numpy as np

CHUNK = 128                       # symbols per chunk of k_dec_tans_ls
TILE = 1536                       # tokens per tile of k_dec_translate
BUCKETS = (12, 13, 14, 15, 16)    # table-size classes: tableLog <= 12, 13, 14, 15, 16
GEOM = {12: (4, 4), 13: (3, 3), 14: (2, 2), 15: (1, 2), 16: (1, 1)}   # bucket -> (streams per wave, waves per group)
BY_GL, BY_SERIAL = 31, 32         # MicUnit.dec_kernel of k_dec_tans_gl / k_dec_tans_serial; 1 + class for k_dec_tans_ls; 0: nobody
MIN_TABLELOG, MAX_TABLELOG = 5, 16


def states(flavour):
    return 8 if flavour == 108 else flavour


def dec_cls(flavour, table_log, zero_bits):
    """mic_dec_cls: the lane-per-state class of a stream, -1 when it is left to k_dec_tans_gl / k_dec_tans_serial"""
    ns = states(flavour)
    if ns not in (2, 4, 8) or not MIN_TABLELOG <= table_log <= MAX_TABLELOG or (table_log == 16 and zero_bits):
        return -1
    return (4 if table_log <= 12 else table_log - 13) * 6 + {2: 0, 4: 2, 8: 4}[ns] + (1 if zero_bits else 0)


def dec_record(flavour, table_log, zero_bits):
    """what MicUnit.dec_kernel must read for a stream of under 2^27 bytes that decodes"""
    c = dec_cls(flavour, table_log, zero_bits)
    return c + 1 if c >= 0 else BY_SERIAL if flavour == 1 else BY_GL


def units_per_batch(bucket):
    """a full group, a full wave of the next group, and a last wave of one stream beside its clones"""
    spw, waves = GEOM[bucket]
    return spw * waves + spw + 1


def min_tokens(table_log):
    """the fewest tokens for which optimal_table_log grants table_log: highbit(n - 1) - 2 >= table_log"""
    return (1 << (table_log + 2)) + 1


def literal_tokens(pixels):
    """tokens of a frame without a run or an escape: the delimiter, then the maximum and a symbol per pixel in literal chunks -- a
    header, and one more for every 124 symbols the tokeniser flushes from its buffer of 126 (rlecompressu16.go:57-67)"""
    return 3 + pixels + max(pixels - 2, 0) // 124


def tail_residues(flavour):
    n = states(flavour)
    return (0, 1, n - 1, n, n + 1, CHUNK - 1)


# ---- images ---------------------------------------------------------------------------------------------------------------
def _mix(n, seed):
    """n 64-bit hashes of (index, seed): splitmix64's finaliser, the same on every numpy"""
    z = np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64((seed * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1))
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _noise(n, seed, amp):
    return ((_mix(n, seed) >> np.uint64(33)) % np.uint64(amp)).astype(np.int64)


def plain_image(w, h, seed, amp):
    """eight bits: a triangle wave along x + 2 y under `amp` levels of noise; no escapes, hardly a run, no dominant token"""
    y, x = np.mgrid[0:h, 0:w]
    tri = np.abs((((x + 2 * y + 7 * seed) >> 2) & 63) - 32)
    return (96 + tri + _noise(w * h, seed, amp).reshape(h, w)).astype(np.uint16)


def dominant_image(w, h, seed, spread=41, alt=0, shift=0):
    """eight bits, one token value on two pixels of three that never makes a run of three: columns come in groups of three at one
    level, so the second and third pixel of a group have their left neighbour's value and predict themselves (residual 0: a level
    steps down by one from row to row at most, and (2 p + 1) >> 1 = p), while the first pixel of a group carries the difference of
    two groups' levels (`alt`: odd groups lie that much higher, so that in a frame of a few rows no two neighbours are level and
    the first pixel never joins the run; `shift` = 2 with w = 3 m + 2: a row opens and closes with a group of one pixel, so the
    residual 0 or -1 of a row's first pixel has no pair of zeros before or behind it -- for frames so narrow that a run per row would
    cost the dominant token its majority).  Nothing reaches the ends of the range: levels stay inside 100 - steps .. 100 + spread + alt."""
    nj = (w - 1 + shift) // 3 + 1
    p0 = 100 + _noise(nj, seed, spread) + alt * (np.arange(nj) & 1)
    per_4096 = min(512, 60 * 4096 // max(h, 1))                          # about sixty steps per group over the frame at most
    step = (_noise(h * nj, seed + 1, 4096) < per_4096).reshape(h, nj)
    step[0] = False
    p = p0[None, :] - np.cumsum(step, axis=0)
    assert p.min() >= 0
    return p[:, (np.arange(w) + shift) // 3].astype(np.uint16)


def deep_image(w, h, seed):
    """sixteen bits, more than 2^18 tokens: a quiet ramp, and two bands of rows (one of them the last rows, the first the bit
    reader meets) whose pixels are uniform over half the range -- no escape (|residual| < 32767), and nearly every token of a band
    a value the frame holds once or twice: 15 or 16 bits each at tableLog 16, a chunk of 128 then takes about 64 dwords off the ring"""
    y, x = np.mgrid[0:h, 0:w]
    img = 20000 + 8 * x + 16 * y + _noise(w * h, seed, 64).reshape(h, w)
    wild = 16384 + (_mix(w * h, seed + 1) >> np.uint64(40)).astype(np.int64).reshape(h, w) % 32768
    band = np.zeros(h, bool)
    band[h // 3: h // 3 + 40] = True
    band[h - 24:] = True
    return np.where(band[:, None], wild, img).astype(np.uint16)


def with_flat_start(img, k):
    if k:
        img = img.copy()
        img[0, :k] = img[0, k]
    return img


def frame_with_tokens(mico, target, make, w=1000):
    """an image make(w, h) of a width just under `w` with the flat start that gives exactly `target` tokens: a flat pixel more is
    about a token less, so a few steps of k += tokens - target get there; a width at which they do not is left for the next"""
    for wt in range(w, w - 60, -1):
        h = max(2, -(-(target * 124 // 125) // wt))
        img = make(wt, h)
        while mico.delta_rle_compress(img, 255).size < target:
            h += 1
            img = make(wt, h)
        k, tried = 0, {}
        for _ in range(8):
            tried[k] = mico.delta_rle_compress(with_flat_start(img, k), 255).size
            if tried[k] == target:
                return with_flat_start(img, k)
            k = min(max(k + tried[k] - target, 0), wt - 1)
            if k in tried:
                break
        k0 = min(tried, key=lambda c: abs(tried[c] - target))
        for k in range(max(k0 - 3, 0), min(k0 + 4, wt)):
            if k not in tried and mico.delta_rle_compress(with_flat_start(img, k), 255).size == target:
                return with_flat_start(img, k)
    raise AssertionError(f"no frame of {target} tokens")


# ---- units and batches ----------------------------------------------------------------------------------------------------
class Stream:
    """one unit: its image, its blob, and what the ORACLE says of the blob"""

    def __init__(self, mico, img, maxv, flavour, req_tl):
        self.img, self.maxv, self.flavour = img, maxv, flavour
        tok = mico.delta_rle_compress(img, maxv)
        self.ntok = int(tok.size)
        self.rc, self.blob = mico.fse_compress_tl(tok, flavour, req_tl)
        frc, f = mico.fse_stream_facts(tok, flavour, req_tl)
        assert self.rc == 0 and frc == 0, (self.rc, frc, img.shape, flavour, req_tl)
        self.table_log, self.zero_bits, self.hdr_len = f["table_log"], f["zero_bits"], f["hdr_len"]
        self.cls = dec_cls(flavour, self.table_log, self.zero_bits)
        self.record = dec_record(flavour, self.table_log, self.zero_bits)

    @property
    def dims(self):
        return self.img.shape[1], self.img.shape[0]


def worst_chunk_dwords(mico, stream, req_tl):
    """the most dwords a whole chunk of 128 tokens of the stream takes off the bit window at the least, from the normalised counts
    the header states: a symbol of count c <= 1 costs tableLog bits in every state, one of count c >= 2 costs tableLog - highbit(c - 1)
    or one bit less, by the state it is met in (build_ctable's maxBitsOut, oracle/mic_oracle_core.c) -- the lesser is taken"""
    tok = mico.delta_rle_compress(stream.img, stream.maxv)
    rc, f = mico.fse_stream_facts(tok, stream.flavour, req_tl, want_norm=True)
    assert rc == 0 and f["table_log"] == stream.table_log
    c = np.maximum(f["norm"].astype(np.int64), 1)
    bits = np.where(c == 1, stream.table_log, stream.table_log - 1 - np.floor(np.log2(np.maximum(c - 1, 1))).astype(np.int64))
    whole = tok.size // CHUNK * CHUNK
    return int(bits[tok[:whole]].reshape(-1, CHUNK).sum(axis=1).max()) / 32


def chunk_plan(bucket, flavour):
    """token counts of a class batch, unit by unit.  Inside a wave every stream has its own number of whole chunks and exactly one
    is the shortest; over the waves of a group that one sits in slot 0, 1, ... in turn.  Tails go round tail_residues().  At
    tableLog 13 and 14 the units whose tail is 127, 0 and 1 are moved up to 1536 k - 1, 1536 k and 1536 k + 1 tokens (k_dec_translate's
    tile; k_dec_translate_wide's vector tail is met by every count that is no multiple of eight)."""
    spw, waves = GEOM[bucket]
    res = tail_residues(flavour)
    first = {12: 0, 13: 0, 14: 0, 15: 1, 16: 4}[bucket]                   # (tableLog 15 and 16 share one round of the six tails: 1 .. 4, then 5, 0)
    base = -(-min_tokens(bucket) // CHUNK)
    plan = []
    for i in range(units_per_batch(bucket)):
        wave, slot = divmod(i, spw)
        r = res[(first + i) % 6]
        chunks = base + (0 if slot == wave % spw else 12 * (1 + slot) + wave % waves)   # (twelve chunks apart: the move to a tile edge below keeps them so)
        if bucket in (13, 14) and r in (0, 1, CHUNK - 1):
            chunks = -(-chunks // 12) * 12 - (1 if r == CHUNK - 1 else 0)
        plan.append(chunks * CHUNK + r)
    return plan


_cache = {}


def class_batch(mico, bucket, flavour, zb):
    """the batch of one class: units_per_batch(bucket) streams (module-level cache: built once per process)"""
    key = (bucket, flavour, zb)
    if key in _cache:
        return _cache[key]
    plan = chunk_plan(bucket, flavour)
    seed0 = 1000 * bucket + 10 * states(flavour) + zb
    units = []
    for i, target in enumerate(plan):
        seed = seed0 * 64 + i
        if zb:
            make = lambda w, h, s=seed: dominant_image(w, h, s)
        else:
            make = lambda w, h, s=seed, a=3 + 5 * (i % 7): plain_image(w, h, s, a)
        units.append(Stream(mico, frame_with_tokens(mico, target, make, 1000 - 13 * (i % 9)), 255, flavour, bucket))
    if bucket == 12:
        # wave 0: four streams of under 128 tokens (no whole chunk in the wave); wave 1: 43 tokens beside thousands; wave 2:
        # tableLog 5, 9 and 12 under one template instance.  Each short stream is its wave's shortest, in the slot whose turn it is.
        small = lambda w, h, s: dominant_image(w, h, s, 3, 8) if zb else plain_image(w, h, s, 3)
        for i, (w, h, tl) in {0: (40, 1, 5), 1: (90, 1, 5), 2: (120, 1, 5), 3: (80, 1, 5),
                              4: (900, 4, 9), 5: (40, 1, 5), 6: (700, 7, 9), 7: (1000, 3, 9),
                              8: (1000, 3, 9), 9: (800, 5, 9), 10: (40, 1, 5)}.items():
            tries = (Stream(mico, small(w, h, seed0 * 64 + i + 1000 * t), 255, flavour, tl) for t in range(50))
            # (a seed at which a frame of one row has no run -- 40 pixels are 43 tokens -- and the table is of the batch's kind)
            units[i] = next(u for u in tries if u.zero_bits == zb and (h > 1 or u.ntok == literal_tokens(w)))
    if bucket == 16 and not zb:
        units[0] = Stream(mico, deep_image(1000, 270, seed0), 65535, flavour, 16)
    _cache[key] = units
    return units


def tiny_batch(mico, n=1100):
    """about 1100 frames of a few hundred pixels for k_dec_classify's passes of 1024: the six classes of tableLog <= 12 and rANS-8
    unit by unit, a 1-state stream every 97th"""
    if "tiny" in _cache:
        return _cache["tiny"]
    kinds = [(2, 0), (4, 1), (8, 0), (2, 1), (4, 0), (8, 1), (108, 0)]
    pool = {}
    for fl, zb in kinds + [(1, 0)]:
        pool[fl, zb] = []
        for v in range(4):
            w, h = 3 * (8 + 2 * v + states(fl) // 2) + 2, 9 + 2 * v
            tries = (Stream(mico, dominant_image(w, h, 50 + v + 100 * t, 3, 8, 2) if zb else plain_image(w, h, 60 + v + 100 * t, 3 + v), 255, fl, 0)
                     for t in range(50))
            pool[fl, zb].append(next(u for u in tries if u.zero_bits == zb))
    units = []
    for i in range(n):
        kind = (1, 0) if i % 97 == 96 else kinds[i % len(kinds)]
        units.append(pool[kind][(i // len(kinds)) % 4])
    _cache["tiny"] = units
    return units


def damaged(stream, way):
    """the stream's blob with its end mark moved (the last byte's top bit is where the bit reader starts: `low` puts it at bit 0,
    `high` at bit 7, or one bit down when it is there already) or with three payload bytes changed (`early`: in the bytes read last, `late`: in those read first)"""
    b = bytearray(stream.blob)
    if way == "low":
        b[-1] = 1 if b[-1] != 1 else 3
    elif way == "high":
        b[-1] = b[-1] | 0x80 if b[-1] < 0x80 else b[-1] >> 1
    else:
        span = len(b) - 1 - stream.hdr_len
        at = stream.hdr_len + (span // 7 if way == "early" else span - span // 7)
        for j, bit in ((0, 0x10), (5, 0x01), (11, 0x40)):
            b[at + j] ^= bit
    assert bytes(b) != stream.blob and b[-1] != 0
    return bytes(b)


DAMAGE = ("low", "high", "early", "late")
