"""mic_hip_wsi_patch_plan (no device): the tiles a batch of same-sized patches touches and the number of patch-tile pieces, against
a brute-force restatement -- mark every pixel of every patch, then collect the tiles and the non-empty patch-tile overlaps."""
import numpy as np
import pytest

from wsi_patch_slides import origins

LEVELS = [(200, 150), (64, 64), (1, 1)]
TILES = [(64, 64), (64, 32)]


def patch_sizes(lw, lh):
    return [(48, 40), (1, 1), (130, 70), (lw + 9, lh + 5)]          # the last: larger than the level


def brute(lw, lh, tw, th, xy, pw, ph):
    tiles_x = (lw + tw - 1) // tw
    tile_of = (np.arange(lh)[:, None] // th) * tiles_x + np.arange(lw)[None, :] // tw
    tiles, pieces = set(), 0
    for x, y in xy:
        mark = np.zeros((lh, lw), dtype=bool)
        mark[max(y, 0): max(y + ph, 0), max(x, 0): max(x + pw, 0)] = True
        mine = np.unique(tile_of[mark])
        pieces += len(mine)
        tiles.update(int(t) for t in mine)
    return sorted(tiles), pieces


@pytest.mark.parametrize("level", LEVELS, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("tile", TILES, ids=lambda v: f"t{v[0]}x{v[1]}")
def test_plan_equals_brute_force(mic, level, tile):
    (lw, lh), (tw, th) = level, tile
    for pw, ph in patch_sizes(lw, lh):
        xy = origins(lw, lh, tw, th, pw, ph)
        want_tiles, want_pieces = brute(lw, lh, tw, th, xy, pw, ph)
        tiles, pieces = mic.wsi_patch_plan(lw, lh, tw, th, xy, pw, ph)
        assert tiles.tolist() == want_tiles and pieces == want_pieces, (pw, ph)
        for one in xy:                                                   # each origin alone, too
            t1, p1 = mic.wsi_patch_plan(lw, lh, tw, th, [one], pw, ph)
            w1, wp1 = brute(lw, lh, tw, th, [one], pw, ph)
            assert t1.tolist() == w1 and p1 == wp1 == len(w1), (pw, ph, one)


def test_patches_outside_the_level_touch_nothing(mic):
    tiles, pieces = mic.wsi_patch_plan(200, 150, 64, 64, [(200, 0), (0, 150), (-48, 0), (0, -40), (5000, 5000)], 48, 40)
    assert tiles.size == 0 and pieces == 0
    tiles, pieces = mic.wsi_patch_plan(200, 150, 64, 64, [], 48, 40)
    assert tiles.size == 0 and pieces == 0


def test_repeated_patches_share_tiles_but_not_pieces(mic):
    tiles, pieces = mic.wsi_patch_plan(200, 150, 64, 64, [(40, 40)] * 5, 48, 40)
    assert tiles.tolist() == [0, 1, 4, 5] and pieces == 20
    tiles, pieces = mic.wsi_patch_plan(200, 150, 64, 64, [(3 + i % 10, 2 + i // 10) for i in range(100)], 48, 40)
    assert tiles.tolist() == [0] and pieces == 100


def test_tile_size_zero_is_the_default_256(mic):
    a = mic.wsi_patch_plan(1000, 700, 0, 0, [(250, 250), (900, 600)], 48, 40)
    b = mic.wsi_patch_plan(1000, 700, 256, 256, [(250, 250), (900, 600)], 48, 40)
    assert a[0].tolist() == b[0].tolist() == [0, 1, 4, 5, 11] and a[1] == b[1] == 5


def test_too_small_a_cap_reports_the_count(mic):
    xy = [(40, 40), (150, 100)]
    want, _ = mic.wsi_patch_plan(200, 150, 64, 64, xy, 48, 40)
    assert want.tolist() == [0, 1, 4, 5, 6, 7, 10, 11]                # two patches, each straddling four tiles
    with pytest.raises(mic.MicError) as e:
        mic.wsi_patch_plan(200, 150, 64, 64, xy, 48, 40, cap=want.size - 1)
    assert e.value.code == mic.MIC_ERR_CAPACITY and e.value.ntiles == want.size
    tiles, _ = mic.wsi_patch_plan(200, 150, 64, 64, xy, 48, 40, cap=want.size)
    assert tiles.tolist() == want.tolist()


@pytest.mark.parametrize("args", [
    (0, 150, 64, 64, 48, 40), (200, 0, 64, 64, 48, 40), (200, 150, -1, 64, 48, 40), (200, 150, 64, -1, 48, 40),
    (200, 150, 64, 64, 0, 40), (200, 150, 64, 64, 48, 0), (200, 150, 64, 64, -3, 40),
])
def test_argument_errors(mic, args):
    lw, lh, tw, th, pw, ph = args
    with pytest.raises(mic.MicError) as e:
        mic.wsi_patch_plan(lw, lh, tw, th, [(0, 0)], pw, ph)
    assert e.value.code == mic.MIC_ERR_ARGS


def test_null_pointers_and_negative_count(mic):
    import ctypes as C
    L = mic.lib()
    nt, npc = C.c_uint64(7), C.c_uint64(7)
    xy = np.zeros(2, dtype=np.int32)
    assert L.mic_hip_wsi_patch_plan(200, 150, 64, 64, xy.ctypes.data, -1, 48, 40, None, 0, C.byref(nt), C.byref(npc)) == mic.MIC_ERR_ARGS
    assert L.mic_hip_wsi_patch_plan(200, 150, 64, 64, None, 1, 48, 40, None, 0, C.byref(nt), C.byref(npc)) == mic.MIC_ERR_ARGS
    assert L.mic_hip_wsi_patch_plan(200, 150, 64, 64, xy.ctypes.data, 1, 48, 40, None, 4, C.byref(nt), C.byref(npc)) == mic.MIC_ERR_ARGS
    # the counts alone: no tile buffer, cap 0
    assert L.mic_hip_wsi_patch_plan(200, 150, 64, 64, xy.ctypes.data, 1, 48, 40, None, 0, C.byref(nt), C.byref(npc)) == mic.MIC_ERR_CAPACITY
    assert (nt.value, npc.value) == (1, 1)
    assert L.mic_hip_wsi_patch_plan(200, 150, 64, 64, xy.ctypes.data, 0, 48, 40, None, 0, C.byref(nt), C.byref(npc)) == mic.MIC_OK
    assert (nt.value, npc.value) == (0, 0)
