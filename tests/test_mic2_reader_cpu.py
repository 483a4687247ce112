"""mic_hip_mic2_reader_open / _info (csrc/mic_mic2_crops.hip) on files the oracle wrote: what open pulls through the callback, what
info reports, and the header, table and callback errors.  No device is needed."""
import ctypes as C
import struct

import numpy as np
import pytest

import mic2_crop_volumes as V


@pytest.fixture(scope="module")
def files(mico, synth):
    vol, maxv = V.volume_12bit(synth)
    out = {}
    for temporal in (False, True):
        rc, data = mico.mic2_compress(vol, maxv, temporal)
        assert rc == 0
        out[temporal] = data
    return vol, out


@pytest.mark.parametrize("temporal", [False, True])
def test_open_reads_the_header_and_the_table_only(mic, files, temporal):
    vol, f = files
    data = f[temporal]
    n, h, w = vol.shape
    src = V.RecordingSource(data)
    with mic.Mic2Reader(src, len(data)) as rd:
        assert src.reads == [(0, 20), (20, 8 * n)]
        assert rd.info() == dict(width=w, height=h, nframes=n, temporal=temporal)
        assert src.reads == [(0, 20), (20, 8 * n)]
    for source in (data, np.frombuffer(data, dtype=np.uint8)):             # bytes and arrays, the length taken from them
        with mic.Mic2Reader(source) as rd:
            assert rd.info() == dict(width=w, height=h, nframes=n, temporal=temporal)
    m = V.Mic2File(data)
    assert (m.w, m.h, m.n, m.temporal) == (w, h, n, temporal)


def _open_code(mic, source, file_len):
    with pytest.raises(mic.MicError) as e:
        mic.Mic2Reader(source, file_len)
    return e.value.code


def test_header_and_table_errors(mic, files):
    data = files[1][False]
    n = files[0].shape[0]
    assert _open_code(mic, b"MIC3" + data[4:], len(data)) == mic.MIC_ERR_CORRUPT          # wrong magic
    src = V.RecordingSource(data)
    assert _open_code(mic, src, 19) == mic.MIC_ERR_CORRUPT and src.reads == []             # shorter than the fixed header
    src = V.RecordingSource(data)
    assert _open_code(mic, src, 20 + 8 * n - 1) == mic.MIC_ERR_CORRUPT                     # the table overruns the file
    assert src.reads == [(0, 20)]
    grown = data[:12] + struct.pack("<I", (len(data) - 20) // 8 + 1) + data[16:]           # ... by the header's own count
    assert _open_code(mic, grown, len(grown)) == mic.MIC_ERR_CORRUPT
    with mic.Mic2Reader(data[: 20 + 8 * n], 20 + 8 * n) as rd:                             # the table fits exactly: fine
        assert rd.info()["nframes"] == n


def test_a_failing_callback_is_an_io_error(mic, files):
    data = files[1][True]
    for fail_at in (0, 1):                                                # the header read, the table read
        calls = []

        def read(user, off, ptr, n):
            calls.append((off, n))
            if len(calls) - 1 == fail_at:
                return 1
            C.memmove(ptr, data[off: off + n], n)
            return 0
        cb = mic._READ_FN(read)
        h = C.c_void_p()
        assert mic.lib().mic_hip_mic2_reader_open(cb, None, len(data), C.byref(h)) == mic.MIC_ERR_IO
        assert not h.value and len(calls) == fail_at + 1

    def broken(off, n):                                                   # through the Python class the source's own exception comes back
        raise OSError("no such sector")
    with pytest.raises(OSError):
        mic.Mic2Reader(broken, len(data))
    null = C.c_void_p()
    assert mic.lib().mic_hip_mic2_reader_open(mic._READ_FN(), None, len(data), C.byref(null)) == mic.MIC_ERR_ARGS
    assert mic.lib().mic_hip_mic2_reader_info(None, None, None, None, None) == mic.MIC_ERR_ARGS
