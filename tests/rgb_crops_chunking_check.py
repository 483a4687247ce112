"""Run by tests/test_gpu_rgb_crops.py in a fresh process whose environment sets MIC_HIP_WS_BUDGET_MB (the ceiling is read once): the RGB
file crop reader's sub-batch seams, and what a slab of coded planes alone buys.  K grey-in-RGB frames (R = G = B: modes [2, 0, 0], one
coded plane each) against K full-colour frames of the same size (three coded planes each); the same crops of both, each against the
numpy crops of its sources; the chains each call ran."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conftest  # noqa: E402
import rgb_crop_files as F  # noqa: E402

K, W, H, CW, CH = 6, 80, 60, 33, 9


def main():
    import torch
    mic = conftest.load_package()
    synth = importlib.import_module("medical_image_codec_amd.synth")
    from oracle import mico
    colour = [synth.wsi_like(W, H, seed=20 + i) for i in range(K)]
    grey = [np.ascontiguousarray(np.repeat(c[..., 1:2], 3, axis=2)) for c in colour]
    slabs = {}
    for name, imgs, coded in (("grey", grey, 1), ("colour", colour, 3)):
        files = []
        for im in imgs:
            rc, blob = mico.wsi_compress_tile(im)
            assert rc == 0 and F.modes(blob).count(2) == coded, (name, rc)
            files.append((im, (blob, W, H), F.modes(blob)))
        entries = [f for _, f, _ in files]
        xyf = F.origins(files, CW, CH)
        file_of, planes, pieces, fs = mic.rgb_crop_plan(entries, xyf, CW, CH)
        assert file_of.tolist() == list(range(K)) and planes == K * coded and not fs.any()
        want = F.expected(files, xyf, CW, CH)
        for _ in range(2):
            t = torch.full((len(xyf), CH, CW, 3), 0xA5, dtype=torch.uint8, device="cuda")
            st, bad, stats = mic.rgb_read_crops(entries, xyf, CW, CH, t.data_ptr(), t.numel())
            assert (st == 0).all() and (bad == -1).all(), (name, st, bad)
            assert np.array_equal(t.cpu().numpy(), want), name
            assert stats["planes_decoded"] == planes and stats["planes_total"] == 3 * K and stats["pieces"] == pieces, (name, stats)
        slabs[name] = stats["slabs"]
    assert slabs["colour"] >= 2 and slabs["grey"] < slabs["colour"], slabs
    print("rgb crop seams ok", slabs)


if __name__ == "__main__":
    main()
