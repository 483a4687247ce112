"""Bare FSE units for the table stage's seams (tests/test_table_routes_cpu.py, tests/test_gpu_table_routes.py).

A case is a histogram, a flavour and a requested tableLog; its symbols are np.repeat of the histogram under a fixed permutation
(synth.hash_u64), so the bitstream is not trivially sorted.  `aim` names the seam the case is there for; the CPU test works the seam
out again from the model of tests/table_routes.py and asserts it, so a case cannot silently stop aiming at it.  Nothing here needs
a device."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import table_routes as M

Case = namedtuple("Case", "name group hist flavour req_tl aim")

TILE = 1024                                                                 # symbols per pass of tb_write_ncount_par


def _hash(n, seed):
    from conftest import load_package
    load_package()
    import importlib
    return importlib.import_module("medical_image_codec_amd.synth").hash_u64(n, seed)


def _counts(k, lo, hi, seed):
    """k pseudo-random counts in [lo, hi]"""
    return (lo + (_hash(k, seed) >> np.uint64(33)).astype(np.int64) % (hi - lo + 1)).astype(np.int64)


def _sparse(length, entries):
    h = np.zeros(length, np.int64)
    for i, c in entries:
        h[i] = c
    return h


def _runs_closing_at_tiles(zs, body=300):
    """zero runs of exactly zs[k] zeros, run k closing on symbol (k + 1) * TILE; a few symbols at the front carry the mass"""
    e = [(i, body - 17 * i) for i in range(6)]
    for k, z in enumerate(zs):
        t = (k + 1) * TILE
        e += [(t - z - 1, 9 + k), (t, 40 + 3 * k)]
    return _sparse(len(zs) * TILE + 1, e)


RUNS_A = (23, 24, 25, 47, 48, 72, 49)                                        # zeros per run: R = zeros - 1 is what the run code counts
RUNS_B = (26, 50, 73, 74, 63, 64, 65)                                        # 24 q + 3 r + {0, 1, 2} + 1 with q = 2, r = 5: 63, 64, 65; ...
WRAP_R = (15, 18)                                                            # [1, 0 x (R + 1), big, 1] at tableLog 16: 15 wraps, 18 does not
STRADDLE_ONES = (5572, 5573)                                                 # ones in front of 50000: headers of 8177 and 8178 bytes


@lru_cache(maxsize=None)
def _all():
    c = []

    def add(name, group, hist, flavours=(2,), req_tl=0, aim=None):
        for f in flavours:
            c.append(Case(f"{name}/{f}" + (f"/tl{req_tl}" if req_tl else ""), group, np.asarray(hist, np.int64), f, req_tl, aim))

    image_like = np.round(6000 * np.exp(-np.arange(300) / 40.0)).astype(np.int64) + 1
    # ---- normaliser -----------------------------------------------------------------------------------------------------------
    add("image-like", "normaliser", image_like, (2, 108), aim=("norm", "PRIMARY"))
    add("40x2000+500x1", "normaliser", [2000] * 40 + [1] * 500, (2, 4), aim=("norm", "N2_PAR"))
    add("4000x3+5000", "normaliser", [3] * 4000 + [5000], (2, 8), aim=("norm", "N2_UNIFORM"))
    add("2800x8", "normaliser", [8] * 2800, (2, 4), aim=("norm", "N2_SERIAL"))
    add("4096x4", "normaliser", [4] * 4096, (2,), aim=("rc", M.ERR_INTERNAL))
    # ---- writer ---------------------------------------------------------------------------------------------------------------
    h = _counts(1030, 5, 60, 11); h[1023] = 0
    add("zero-1023-closed-1024", "writer", h, aim=("run", 1023, 1024))
    add("run-over-a-whole-tile", "writer", _sparse(2200, [(i, 5 + i % 50) for i in range(1000)] + [(2100 + i, 50 + i) for i in range(100)]),
        aim=("run", 1000, 2100))
    h = _counts(400, 5, 60, 12); h[383] = 0
    add("zero-lane63-closed-lane0", "writer", h, aim=("run", 383, 384))
    add("runs-at-tile-borders-a", "writer", _runs_closing_at_tiles(RUNS_A), aim=("tile-runs", RUNS_A))
    add("runs-at-tile-borders-b", "writer", _runs_closing_at_tiles(RUNS_B), aim=("tile-runs", RUNS_B))
    add("runs-at-tile-borders-hbm", "writer", _runs_closing_at_tiles(RUNS_A + RUNS_B), aim=("tile-runs", RUNS_A + RUNS_B))
    add("ones-over-three-words", "writer", _sparse(140, [(0, 90), (1, 31), (2, 22), (3, 13), (103, 7), (104, 9)]), aim=("three-words",))
    add("header-ends-on-bit-7", "writer", [40, 30, 20, 10, 5, 3], aim=("last-bit", 0))
    add("header-ends-on-bit-0", "writer", [40, 30, 20, 10, 5, 3, 2, 14], aim=("last-bit", 1))
    add("tl16-parallel-writer", "writer", [1] + [0] * (WRAP_R[1] + 1) + [300000, 1], req_tl=16, aim=("wrap", False))
    add("tl16-field-wraps", "writer", [1] + [0] * (WRAP_R[0] + 1) + [300000, 1], req_tl=16, aim=("wrap", True))
    # ---- scratch class --------------------------------------------------------------------------------------------------------
    add("alphabet-8192-tl13", "scratch", _sparse(8192, [(i, 1 + i % 3) for i in range(0, 8190, 2)] + [(8191, 40000)]), (2, 108),
        aim=("scratch", 8192, 13, "SMALL"))
    add("alphabet-8193-tl13", "scratch", _sparse(8193, [(i, 1 + i % 3) for i in range(0, 8190, 2)] + [(8192, 40000)]), (2, 108),
        aim=("scratch", 8193, 13, "HBM"))
    add("sparse-alphabet-9001-tl10", "scratch", _sparse(9001, [(i, 400 - 19 * i) for i in range(20)] + [(9000, 77)]), aim=("scratch", 9001, 10, "HBM"))
    geo = np.round(1150 * np.exp(-np.arange(600) / 70.0)).astype(np.int64) + 2         # n in (65536, 131072): tableLog 14 can be asked for
    add("small-alphabet", "scratch", geo, (2, 108), req_tl=13, aim=("scratch", 600, 13, "SMALL"))
    add("small-alphabet", "scratch", geo, (2, 108), req_tl=14, aim=("scratch", 600, 14, "HBM"))
    add("9001-symbols", "scratch", list(np.arange(9000) % 40 + 1) + [5823], req_tl=15, aim=("scratch", 9001, 15, "HBM"))
    add("near-full-alphabet", "scratch", [200000] + list(np.arange(65535) % 4), (2, 108), req_tl=16, aim=("scratch", 65536, 16, "HBM"))
    # ---- spread ---------------------------------------------------------------------------------------------------------------
    add("one-bitmap-word", "spread", [40, 30, 20, 10, 5, 3], (1, 2, 4, 8, 108), aim=("spread", 5, "low"))
    add("no-low-symbol", "spread", [40, 30, 20, 10, 8], (2, 108), aim=("spread", 5, "nolow"))
    add("slots-1-2-16-17-64-65", "spread", [11, 17, 130, 138, 518, 526, 730], (1, 2, 4, 8, 108), req_tl=8, aim=("slots", (1, 2, 16, 17, 64, 65)))
    add("40-big-symbols", "spread", [2000] * 40 + [1] * 500, (2, 108), aim=("nbig", 13, 40))
    add("481x17-slots", "spread", [100] * 481, (1, 2, 4, 8, 108), req_tl=13, aim=("nbig", 13, 481))
    add("big-symbols-hbm", "spread", geo, (2, 108), req_tl=14, aim=("nbig-hbm", 14))
    add("big-symbols-hbm", "spread", [120000, 90000, 50000, 20000, 9000, 5000, 3000, 700, 40, 3], (2, 108), req_tl=16, aim=("nbig-hbm", 16))
    # ---- parse ----------------------------------------------------------------------------------------------------------------
    add("header-8177", "parse", [1] * STRADDLE_ONES[0] + [50000], aim=("straddle", 8177, "P_SMALL"))
    add("header-8178", "parse", [1] * STRADDLE_ONES[1] + [50000], aim=("straddle", 8178, "P_DEFER_LEN"))
    add("tl16-short-header-long-blob", "parse", [60000, 50000, 45000, 40000, 35000, 30000, 25000, 15000], req_tl=16, aim=("big", "P_BIG_STAGE"))
    add("tl16-long-header", "parse", [200000] + list(np.arange(65535) % 4), req_tl=16, aim=("big", "P_BIG_HBM"))
    add("sparse-alphabet-9001-short-blob", "parse", _sparse(9001, [(i, 400 - 19 * i) for i in range(20)] + [(9000, 77)]), aim=("defer", "P_DEFER_SYMS"))
    add("under-24-bytes", "parse", [5, 4, 3], (1, 2), aim=("tail", "no-window"))
    add("under-24-bytes-b", "parse", [10, 5, 3, 2, 1, 1], (1, 2, 8), aim=("tail", "no-window"))
    add("ffff-and-header-end-in-the-last-16", "parse", [30, 1, 1, 1] + [0] * (24 * 8 + 1) + [1, 1], aim=("tail", "inside-16+bail"))
    add("header-ends-16-from-the-end", "parse", [26, 30, 2, 1] + [0] * (24 * 4 + 1) + [1, 6], aim=("tail", "exactly-16"))
    # ---- gates, between units that succeed --------------------------------------------------------------------------------------
    ok = [40, 30, 20, 10, 5, 3]
    add("ok-a", "gates", ok, aim=("rc", 0))
    add("max-is-n", "gates", [0, 0, 50], aim=("rc", M.ERR_USE_RLE))
    add("ok-b", "gates", image_like, aim=("rc", 0))
    add("max-is-1", "gates", [1] * 50, aim=("rc", M.ERR_INCOMPRESSIBLE))
    add("ok-c", "gates", [2000] * 40 + [1] * 500, (4,), aim=("rc", 0))
    add("max-under-n>>15", "gates", [2] * 50000, aim=("rc", M.ERR_INCOMPRESSIBLE))
    add("ok-d", "gates", [8] * 2800, (8,), aim=("rc", 0))
    add("n-under-lanes", "gates", [1], (2,), aim=("rc", M.ERR_INCOMPRESSIBLE))
    add("ok-e", "gates", ok, (4,), aim=("rc", 0))
    add("n-under-lanes", "gates", [2, 1], (4,), aim=("rc", M.ERR_INCOMPRESSIBLE))
    add("ok-f", "gates", ok, (8,), aim=("rc", 0))
    add("n-under-lanes", "gates", [4, 3], (8,), aim=("rc", M.ERR_INCOMPRESSIBLE))
    add("ok-g", "gates", ok, (108,), aim=("rc", 0))
    add("n-under-lanes", "gates", [4, 3], (108,), aim=("rc", M.ERR_INCOMPRESSIBLE))
    add("ok-h", "gates", ok, (1,), aim=("rc", 0))
    add("4096x4-between", "gates", [4] * 4096, aim=("rc", M.ERR_INTERNAL))
    add("ok-i", "gates", [3] * 4000 + [5000], aim=("rc", 0))
    return tuple(c)


GROUPS = ("normaliser", "writer", "scratch", "spread", "parse", "gates")


def group(name):
    return [c for c in _all() if c.group == name]


def cases():
    return list(_all())


@lru_cache(maxsize=None)
def _symbols(key):
    case = next(c for c in _all() if c.name == key)
    sym = np.repeat(np.arange(case.hist.size), case.hist).astype(np.uint16)
    return sym[np.argsort(_hash(sym.size, 7), kind="stable")]


def symbols(case):
    return _symbols(case.name)


@lru_cache(maxsize=None)
def _unit(key):
    case = next(c for c in _all() if c.name == key)
    return M.Unit(case.hist, case.flavour, case.req_tl)


def unit(case):
    """the model's account of the case (tests/table_routes.py), computed once"""
    return _unit(case.name)


_REF = {}


def reference(mico, case):
    """the oracle's account of the case, computed once: (rc, facts with `norm`, blob)"""
    if case.name not in _REF:
        sym = symbols(case)
        rc, facts = mico.fse_stream_facts(sym, case.flavour, case.req_tl, want_norm=True)
        rc2, blob = mico.fse_compress_tl(sym, case.flavour, case.req_tl)
        assert rc == rc2, (case.name, rc, rc2)
        _REF[case.name] = (rc, facts, blob)
    return _REF[case.name]
