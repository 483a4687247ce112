"""k_dec_rows_tok (csrc/mic_decode_fused.hip) runs one wave per unit, several units per block: batches whose unit counts are below,
at and beyond a block's units -- 1, 2, 3, 4, 5 and 7 strips of the headline's width (2577 columns, 8 .. 16 rows) -- so that the last
block holds every number of live waves, whatever the block's shape.  The pixels are the source's, and MicUnit.dec_stage
(mic_hip_debug_dec_stage) shows that the fused kernel, not the two kernels under it, made every unit's pixels."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STAGE_PIXELS = 4                           # MIC_STAGE_PIXELS (csrc/mic_dev.h)
W = 2577


def _stage(mic, sess, i):
    r = C.c_uint32()
    L = mic.lib()
    L.mic_hip_debug_dec_stage.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    assert L.mic_hip_debug_dec_stage(sess._h, i, C.byref(r)) == 0
    return int(r.value)


@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 7))
def test_every_unit_of_a_short_batch_is_decoded_by_the_fused_kernel(mic, synth, gpu_ready, n):
    torch = pytest.importorskip("torch")
    frame = synth.xr_like(cols=W, rows=128, depth=12, seed=40 + n)
    rows = [8 + (3 * i) % 9 for i in range(n)]                               # 8 .. 16 rows
    strips = [np.ascontiguousarray(frame[8 * i:8 * i + r]) for i, r in enumerate(rows)]
    host = np.concatenate([s.ravel() for s in strips])
    off = np.concatenate([[0], np.cumsum([s.size for s in strips])])
    d_px = torch.from_numpy(host.view(np.int16)).cuda()
    d_out = torch.zeros_like(d_px)
    units = mic.Session.make_units([(int(off[i]), W, rows[i], 4095, 2) for i in range(n)])
    sess = mic.Session(n, W * 16)
    try:
        sess.encode_enqueue(d_px.data_ptr(), units)
        d_blobs, offs, st, _ = sess.encode_finish()
        assert (np.asarray(st) == 0).all()
        sess.decode_enqueue(d_blobs, offs, units, d_out.data_ptr())
        dst = sess.decode_finish()
        assert (np.asarray(dst) == 0).all()
        assert torch.equal(d_out, d_px)
        assert [_stage(mic, sess, i) for i in range(n)] == [STAGE_PIXELS] * n
    finally:
        sess.close()
