"""The one greedy cut of a unit list into sub-batches (next_sub_batch, csrc/mic_staged.h) without a device, through a debug door that
is not in the public header (mic_hip_debug_cuts, csrc/mic_host_io.hip).  The test states the capacity itself, as a step function
of the largest item, so nothing here depends on a memory figure.  Every cut is compared with the five loops the cutter replaced,
restated below one small function each from the sources they stood in: next_cut<U> and the PICA strip pairs (mic_host_io.hip),
rgb_next_cut (mic_rgb_batch.hip), next_strip_cut (mic_strip_crops.hip) and the tile loop of read_patches (mic_api_ext.hip)."""
import ctypes as C
import random

import numpy as np
import pytest

NONE = (1 << 64) - 1                                     # no limit / no target
RGB_MAX_IMAGES = 65535 // 3                              # kRgbMaxImages; also kMaxGridY / P for three-plane tiles


def units(tab, mp):
    """the step function: the first row whose px >= mp holds, the last row beyond it"""
    for px, u in tab[:-1]:
        if px >= mp:
            return u
    return tab[-1][1]


def door(mic, px, tab, per=1, limit=NONE, item_target=NONE, px_target=NONE, flag=None, tab_flag=None):
    L = mic.lib()
    L.mic_hip_debug_cuts.restype = C.c_int
    L.mic_hip_debug_cuts.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                     C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint64)]
    p = np.ascontiguousarray(px, np.uint64)
    t = np.ascontiguousarray(tab, np.uint64).reshape(-1, 2)
    f = None if flag is None else np.ascontiguousarray(flag, np.uint8)
    tf = None if tab_flag is None else np.ascontiguousarray(tab_flag, np.uint64).reshape(-1, 2)
    cuts = np.zeros(len(p) + 2, np.uint64)
    nc = C.c_uint64()
    rc = L.mic_hip_debug_cuts(p.ctypes.data, None if f is None else f.ctypes.data, len(p), t.ctypes.data, len(t),
                              None if tf is None else tf.ctypes.data, 0 if tf is None else len(tf),
                              per, limit, item_target, px_target, cuts.ctypes.data, len(cuts), C.byref(nc))
    assert rc == 0, rc
    return cuts[:nc.value].tolist()


def _all(n, one):
    cuts = [0]
    while cuts[-1] < n:
        cuts.append(one(cuts[-1]))
    return cuts


# ---- the five loops of the parent commit, restated --------------------------------------------------------------------------

def parent_next_cut(px, flag, tab, tab_flag, target):
    """next_cut<U>: extra = 12 mp + the gap slab, a unit target, 65535"""
    n = len(px)

    def one(i0):
        max_px = cap = gap_x = 0
        i1 = i0
        while i1 < n:
            mp = max(max_px, px[i1])
            gx = max(gap_x, 1 if flag[i1] else 0)
            if mp != max_px or gx != gap_x or cap == 0:
                cap = units(tab_flag if gx else tab, mp)
            gap_x = gx
            if i1 > i0 and (i1 - i0 + 1 > cap or i1 - i0 >= target or i1 - i0 >= 65535):
                break
            max_px = mp
            i1 += 1
        return i1
    return _all(n, one)


def parent_pica_cut(px, tab):
    """pica_encode_run: two units per strip, 65534"""
    n = len(px)

    def one(s0):
        max_px = cap = 0
        s1 = s0
        while s1 < n:
            mp = max(max_px, px[s1])
            if mp != max_px or cap == 0:
                cap = units(tab, mp)
            if s1 > s0 and (2 * (s1 - s0 + 1) > cap or 2 * (s1 - s0 + 1) > 65534):
                break
            max_px = mp
            s1 += 1
        return s1
    return _all(n, one)


def parent_rgb_cut(px, tab, target_px):
    """rgb_next_cut: three units per image, a pixel target, kRgbMaxImages"""
    n = len(px)

    def one(i0):
        max_px = cap = tot = 0
        i1 = i0
        while i1 < n:
            p = px[i1]
            mp = max(max_px, p)
            if mp != max_px or cap == 0:
                cap = units(tab, mp)
            cnt = i1 - i0
            if cnt > 0 and (3 * (cnt + 1) > cap or tot >= target_px or cnt >= RGB_MAX_IMAGES):
                break
            max_px = mp
            tot += p
            i1 += 1
        return i1
    return _all(n, one)


def parent_strip_cut(px, tab):
    """next_strip_cut: budget / (unit_ws_bytes(mp) + 2 mp) is the table here, 65535"""
    n = len(px)

    def one(i0):
        max_px = 0
        i1 = i0
        while i1 < n:
            mp = max(max_px, px[i1])
            if i1 > i0 and (i1 - i0 + 1 > units(tab, mp) or i1 - i0 >= 65535):
                break
            max_px = mp
            i1 += 1
        return i1
    return _all(n, one)


def parent_tile_cut(px, tab, planes):
    """read_patches: the ceiling is min(kMaxGridY / P, the table), no other limit"""
    n = len(px)

    def one(i0):
        mp = 0
        i1 = i0
        while i1 < n:
            m2 = max(mp, px[i1])
            if i1 > i0 and i1 - i0 + 1 > min(65535 // planes, units(tab, m2)):
                break
            mp = m2
            i1 += 1
        return i1
    return _all(n, one)


def ceiling(tab, planes):
    return [(px, min(65535 // planes, u)) for px, u in tab]


# the five rules as the call sites now state them to the cutter
def new_next_cut(mic, px, flag, tab, tab_flag, target):
    return door(mic, px, tab, 1, 65535, target, NONE, flag, tab_flag)


def new_pica_cut(mic, px, tab):
    return door(mic, px, tab, 2, 65534 // 2)


def new_rgb_cut(mic, px, tab, target_px):
    return door(mic, px, tab, 3, RGB_MAX_IMAGES, NONE, target_px)


def new_strip_cut(mic, px, tab):
    return door(mic, px, tab, 1, 65535)


def new_tile_cut(mic, px, tab, planes):
    return door(mic, px, ceiling(tab, planes), 1, NONE)


def both(mic, px, tab, target=NONE, target_px=NONE, flag=None, tab_flag=None):
    """every rule on one list: each equal to its parent loop; -> the cuts by rule"""
    fl = [0] * len(px) if flag is None else flag
    tf = tab if tab_flag is None else tab_flag
    got = {
        "units": new_next_cut(mic, px, fl, tab, tf, target), "pica": new_pica_cut(mic, px, tab), "rgb": new_rgb_cut(mic, px, tab, target_px),
        "strips": new_strip_cut(mic, px, tab), "tiles1": new_tile_cut(mic, px, tab, 1), "tiles3": new_tile_cut(mic, px, tab, 3),
    }
    want = {
        "units": parent_next_cut(px, fl, tab, tf, target), "pica": parent_pica_cut(px, tab), "rgb": parent_rgb_cut(px, tab, target_px),
        "strips": parent_strip_cut(px, tab), "tiles1": parent_tile_cut(px, tab, 1), "tiles3": parent_tile_cut(px, tab, 3),
    }
    assert got == want
    for c in got.values():
        assert c[0] == 0 and c[-1] == len(px) and all(b > a for a, b in zip(c, c[1:]))
    return got


# ---- the seams ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [0, 1])
def test_an_item_that_exceeds_the_capacity_alone_is_a_sub_batch_of_one(mic, cap):
    got = both(mic, [100, 100, 100], [(1000, cap)])
    assert all(c == [0, 1, 2, 3] for c in got.values())
    assert door(mic, [], [(1, cap)]) == [0]


def test_a_count_that_fills_the_capacity_and_one_more(mic):
    assert both(mic, [9] * 4, [(9, 4)])["strips"] == [0, 4]
    assert both(mic, [9] * 5, [(9, 4)])["strips"] == [0, 4, 5]
    assert both(mic, [9] * 8, [(9, 4)])["units"] == [0, 4, 8]


def test_an_item_that_lowers_the_capacity_below_the_count_opens_the_next_sub_batch(mic):
    tab = [(10, 5), (100, 2)]
    got = both(mic, [10, 10, 10, 100, 10], tab)
    assert got["strips"] == got["units"] == got["tiles1"] == [0, 3, 5]          # three small ones, then the large one and its neighbour
    assert both(mic, [10, 100, 10, 10], tab)["strips"] == [0, 2, 4]             # as the second item it still fits, and ends the sub-batch
    assert both(mic, [10, 10, 100, 100], tab)["strips"] == [0, 2, 4]            # two are taken, two are allowed: it opens the next one too


def test_two_and_three_units_per_item_under_a_capacity_that_is_no_multiple(mic):
    got = both(mic, [5] * 7, [(5, 7)])
    assert got["pica"] == [0, 3, 6, 7]                                          # 7 units: three pairs
    assert got["rgb"] == [0, 2, 4, 6, 7]                                        # ... two images
    got = both(mic, [5] * 3, [(5, 5)])
    assert got["pica"] == [0, 2, 3] and got["rgb"] == [0, 1, 2, 3]


@pytest.mark.parametrize("rule,limit", [("units", 65535), ("strips", 65535), ("pica", 32767), ("rgb", 21845), ("tiles3", 21845), ("tiles1", 65535)])
def test_each_limit_crossed_by_one_item(mic, rule, limit):
    big = [(1, 1 << 40)]
    assert both(mic, [1] * limit, big)[rule] == [0, limit]
    assert both(mic, [1] * (limit + 1), big)[rule] == [0, limit, limit + 1]


def test_a_unit_target_met_exactly_and_a_pixel_target_reached_inside_an_item(mic):
    big = [(100, 1 << 40)]
    assert both(mic, [7] * 6, big, target=3)["units"] == [0, 3, 6]
    assert both(mic, [7] * 7, big, target=3)["units"] == [0, 3, 6, 7]
    assert both(mic, [5] * 4, big, target_px=12)["rgb"] == [0, 3, 4]            # 10 < 12 <= 15: the third image crosses it and stays
    assert both(mic, [5] * 4, big, target_px=10)["rgb"] == [0, 2, 4]            # met exactly
    assert both(mic, [50, 1, 1], big, target_px=12)["rgb"] == [0, 1, 3]         # the first image always joins


def test_a_capacity_that_depends_on_a_second_running_maximum(mic):
    """as next_cut's gap slab: from the first flagged unit on the sub-batch holds fewer, whatever the sizes"""
    tab, tab_flag = [(10, 6), (100, 4)], [(10, 3), (100, 2)]
    px = [10] * 9
    assert both(mic, px, tab)["units"] == [0, 6, 9]
    assert both(mic, px, tab, flag=[0, 0, 0, 0, 1, 0, 0, 0, 0], tab_flag=tab_flag)["units"] == [0, 4, 7, 9]   # cut in front of the flagged unit
    assert both(mic, px, tab, flag=[0, 0, 1, 0, 0, 0, 0, 0, 0], tab_flag=tab_flag)["units"] == [0, 3, 9]      # it still fits: the sub-batch ends behind it
    assert both(mic, [10, 10, 100, 10], tab, flag=[0, 1, 0, 0], tab_flag=tab_flag)["units"] == [0, 2, 4]      # both maxima grow


def test_random_lists_cut_as_the_parent_loops_cut_them(mic):
    """200 seeded lists, each through all five rules (tiles with one plane and with three)"""
    rnd = random.Random(20261019)
    for _ in range(200):
        n = rnd.randint(0, 60)
        sizes = sorted(rnd.sample(range(1, 5000), rnd.randint(1, 5)))
        px = [rnd.choice(sizes) if rnd.random() < 0.8 else rnd.randint(1, 6000) for _ in range(n)]
        caps = sorted((rnd.randint(0, 24) for _ in sizes), reverse=True) if rnd.random() < 0.8 else [rnd.randint(0, 24) for _ in sizes]
        tab = list(zip(sizes, caps))
        tab_flag = [(s, c // 2) for s, c in tab]
        flag = [int(rnd.random() < 0.1) for _ in range(n)]
        target = rnd.choice([NONE, NONE, rnd.randint(1, 12)])
        target_px = rnd.choice([NONE, NONE, rnd.randint(1, 20000)])
        both(mic, px, tab, target, target_px, flag, tab_flag)


def test_the_doors_own_arguments(mic):
    L = mic.lib()
    door(mic, [1], [(1, 1)])                                                    # (sets the argument types)
    one = np.array([1, 1], np.uint64)
    nc = C.c_uint64()
    assert L.mic_hip_debug_cuts(one.ctypes.data, None, 1, one.ctypes.data, 0, None, 0, 1, 1, 1, 1, None, 0, C.byref(nc)) == mic.MIC_ERR_ARGS
    assert L.mic_hip_debug_cuts(one.ctypes.data, None, 1, one.ctypes.data, 1, None, 0, 0, 1, 1, 1, None, 0, C.byref(nc)) == mic.MIC_ERR_ARGS
    assert L.mic_hip_debug_cuts(one.ctypes.data, None, 1, one.ctypes.data, 1, None, 0, 1, 1, 1, 1, None, 0, C.byref(nc)) == mic.MIC_ERR_CAPACITY
    assert nc.value == 2
