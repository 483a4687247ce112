"""What tests/test_gpu_decode_classes.py takes for granted, checked without a device: the oracle's stream facts, the Python
restatement of mic_dec_cls against the library's sources, and the stream builder's promises (tests/decode_class_streams.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import decode_class_streams as D

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "medical-image-codec_amd", "csrc")


def _define(text, name):
    return int(re.search(r"#define\s+%s\s+\(?(-?\d+)" % name, text).group(1))


def test_the_python_class_function_is_the_librarys(mic):
    """value by value against what the library compiled from csrc/mic_launch.h and csrc/mic_decode_ls.hip (two probes that are
    not in the public header; loading the library needs no device)"""
    launch = open(os.path.join(CSRC, "mic_launch.h")).read()
    dev = open(os.path.join(CSRC, "mic_dev.h")).read()
    ls = open(os.path.join(CSRC, "mic_decode_ls.hip")).read()
    assert _define(dev, "MIC_MIN_TABLELOG") == D.MIN_TABLELOG and _define(dev, "MIC_MAX_TABLELOG") == D.MAX_TABLELOG
    assert _define(dev, "MIC_DEC_BY_GL") == D.BY_GL and _define(dev, "MIC_DEC_BY_SERIAL") == D.BY_SERIAL
    ncls = _define(launch, "MIC_CLS_CLASSES")
    assert ncls + 1 == D.BY_GL
    assert _define(launch, "MIC_ROWS_LO") == 1008                            # the widest frame of the GPU module stays under it
    assert (_define(ls, "TR_THREADS") - 64) * 8 == D.TILE
    lib = mic.lib()
    lib.mic_hip_debug_dec_cls.restype = C.c_int
    lib.mic_hip_debug_dec_cls.argtypes = [C.c_uint32] * 3
    seen = set()
    for fl in (0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 107, 108, 109):               # (every gate: the states, the tableLog range, 16 with 0-bit entries)
        for tl in range(0, 20):
            for zb in (0, 1):
                want = lib.mic_hip_debug_dec_cls(fl, tl, zb)
                assert D.dec_cls(fl, tl, zb) == want, (fl, tl, zb)
                seen.add(want)
    assert seen == set(range(ncls)) - {19, 21, 23} | {-1}                    # 27 kernels; tableLog 16 with 0-bit entries has none
    # the geometry: streams per wave and waves per group, as LsGeom states them
    for b in D.BUCKETS:
        spw, waves = C.c_int(), C.c_int()
        assert lib.mic_hip_debug_ls_geom(b, C.byref(spw), C.byref(waves)) == 1
        assert D.GEOM[b] == (spw.value, waves.value), b
    assert [D.units_per_batch(b) for b in D.BUCKETS] == [21, 13, 7, 4, 3]


@pytest.mark.parametrize("pixels,table_log", [(40, 5), (3000, 9), (20000, 12), (40000, 13), (70000, 14), (140000, 15), (270000, 16)])
def test_a_requested_table_log_is_granted_when_the_token_count_allows_it(mico, pixels, table_log):
    img = D.plain_image(pixels, 1, 7, 3)
    tok = mico.delta_rle_compress(img, 255)
    assert tok.size >= D.min_tokens(table_log) or table_log == 5
    for fl in (2, 4, 8, 108):
        rc, blob = mico.fse_compress_tl(tok, fl, table_log)
        frc, f = mico.fse_stream_facts(tok, fl, table_log)
        assert rc == 0 and frc == 0
        assert f["table_log"] == table_log == (blob[6] & 15) + D.MIN_TABLELOG   # (the NCount header opens with tableLog - 5 in four bits)
        assert f["zero_bits"] == 0 and 6 < f["hdr_len"] < len(blob)
        rc, back = mico.decompress_single_frame(blob, pixels, 1)
        assert rc == 0 and np.array_equal(back, img)
    rc1, blob1 = mico.fse_compress_tl(tok, 1, table_log)                    # 1-state: no prefix in front of the header
    frc, f1 = mico.fse_stream_facts(tok, 1, table_log)
    assert rc1 == 0 and frc == 0 and f1["hdr_len"] == f["hdr_len"] - 6 and f1["table_log"] == table_log
    # one tableLog more than the count allows is not granted
    if table_log < 16 and table_log > 5:
        assert mico.fse_stream_facts(tok[: D.min_tokens(table_log) - 1], 2, table_log)[1]["table_log"] == table_log - 1


def test_stream_facts_fail_where_the_encoder_fails(mico):
    assert mico.fse_stream_facts(np.full(500, 9, np.uint16), 2, 0)[0] == mico.ERR_USE_RLE == mico.fse_compress_tl(np.full(500, 9, np.uint16), 2, 0)[0]
    ramp = np.arange(4000, dtype=np.uint16)
    assert mico.fse_stream_facts(ramp, 4, 0)[0] == mico.ERR_INCOMPRESSIBLE == mico.fse_compress_tl(ramp, 4, 0)[0]
    assert mico.fse_stream_facts(ramp[:3], 8, 0)[0] == mico.ERR_INCOMPRESSIBLE
    assert mico.fse_stream_facts(ramp, 2, 17)[0] == mico.ERR_ARGS


@pytest.mark.parametrize("bucket", D.BUCKETS)
def test_a_dominant_token_gives_zero_bit_entries_in_every_bucket(mico, bucket):
    img = D.dominant_image(1000, D.min_tokens(bucket) // 900 + 2, 3)                 # (a tenth to spare: a level pair now and then makes a run)
    for fl in (2, 4, 8, 108):
        s = D.Stream(mico, img, 255, fl, bucket)
        assert s.rc == 0 and s.table_log == bucket and s.zero_bits == 1
        assert s.cls == (-1 if bucket == 16 else D.dec_cls(fl, bucket, 1)) and s.record == (D.BY_GL if bucket == 16 else s.cls + 1)
        tok = mico.delta_rle_compress(img, 255)
        vals, cnt = np.unique(tok, return_counts=True)
        assert cnt.max() * 2 > tok.size and vals[cnt.argmax()] == 127          # residual 0 on more than half of the tokens
        rc, back = mico.decompress_single_frame(s.blob, *s.dims)
        assert rc == 0 and np.array_equal(back, img)
    small = D.Stream(mico, D.dominant_image(40, 1, 5, 3, 8), 255, 2, 5)
    assert (small.ntok, small.table_log, small.zero_bits) == (43, 5, 1)


@pytest.mark.parametrize("flavour", [2, 4, 8])
def test_the_sixteen_bit_frame_has_a_chunk_that_takes_a_whole_ring_block(mico, flavour):
    """tableLog 16 at 16 bits a symbol: 128 symbols are 64 dwords, the bit-window ring's worst case (k_dec_tans_ls, LsGeom<16>)"""
    s = D.Stream(mico, D.deep_image(1000, 270, 16000 + 10 * flavour), 65535, flavour, 16)
    assert (s.rc, s.table_log, s.zero_bits) == (0, 16, 0) and s.ntok > 262144
    assert D.worst_chunk_dwords(mico, s, 16) >= 63
    quiet = D.Stream(mico, D.plain_image(1000, 270, 7, 3), 255, flavour, 16)
    assert quiet.table_log == 16 and D.worst_chunk_dwords(mico, quiet, 16) < 40     # (the measure tells the two apart)


def test_token_counts_are_met_exactly(mico):
    for target, zb in ((33791, 0), (33792, 1), (33793, 0), (16512 + 9, 1)):
        make = (lambda w, h: D.dominant_image(w, h, 11)) if zb else (lambda w, h: D.plain_image(w, h, 11, 9))
        img = D.frame_with_tokens(mico, target, make)
        assert mico.delta_rle_compress(img, 255).size == target and img.shape[1] <= 1008


def test_the_oracle_gives_a_verdict_on_every_damaged_stream(mico):
    verdicts = set()
    for zb in (0, 1):
        s = D.class_batch(mico, 13, 2, zb)[8]
        for way in D.DAMAGE:
            rc, px = mico.decompress_single_frame(D.damaged(s, way), *s.dims)
            assert rc in (0, mico.ERR_CORRUPT), (zb, way, rc)
            verdicts.add(rc)
    assert mico.ERR_CORRUPT in verdicts
