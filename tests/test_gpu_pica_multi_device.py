"""PICA batches over mic_hip_set_devices: the images are cut into one contiguous range per listed device (mic_hip_shard_plan,
weight = pixels) and the files are the one-device files, byte for byte.  As in tests/test_gpu_multi_device.py the lists are {0},
{0, 0} and {0, 0, 0}: the same code path with two and three sessions of one device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture
def device_lists(mic, gpu_ready):
    yield ([0], [0, 0], [0, 0, 0])
    mic.set_devices([0])


def test_pica_batches_over_device_lists_equal_the_oracle(mic, mico, synth, device_lists):
    shapes = [(322, 256), (257, 200), (640, 130), (129, 77), (322, 256), (500, 164), (601, 403), (322, 256), (96, 300), (322, 256), (2577, 64)]
    imgs = [synth.xr_like(cols=w, rows=h, depth=12, seed=700 + i) for i, (w, h) in enumerate(shapes)]
    want = [mico.pica_compress(im, 4095, 4) for im in imgs]
    assert sum(rc == 0 for rc, _ in want) >= 7
    first = None
    for devs in device_lists:
        mic.set_devices(devs)
        assert mic.shard_plan([im.size for im in imgs], len(devs))[-1] == len(imgs)
        res = mic.compress_parallel_strips_adaptive_batch(imgs, 4095, 4)
        files, ok = [], []
        for im, (st, blob), (rc, f) in zip(imgs, res, want):
            assert st == rc, devs                      # (a thin noisy strip neither predictor can code fails its job on any shard)
            if rc == 0:
                assert blob.tobytes() == f, devs
                files.append(f); ok.append(im)
        got = [(st, blob.tobytes()) for st, blob in res]
        first = first or got
        assert got == first, devs                      # the one-device files, byte for byte
        back = mic.decompress_parallel_strips_adaptive_batch(files, [(im.shape[1], im.shape[0]) for im in ok])
        for im, (st, px) in zip(ok, back):
            assert st == 0 and np.array_equal(px, im), devs
