"""Gap removal on CT: 256 frames of the reference's 16-bit CT test image (512 x 512, shifted copies) through a device-resident
session, as plain units and as MIC_HIP_GAP_REMOVAL units, each on a fresh session.  Prints the ratio, the per-kernel
milliseconds of one encode and one decode (the third of three passes: the decode class mask is learned from earlier batches), the
FSE tableLog, and the tANS decode kernels that did the work -- read from the per-kernel timings (a kernel whose launch found no
units of its class costs a few microseconds; one that decoded streams, milliseconds).  Last, a session that has seen only plain
batches meets gap ones: its first gap batch falls through to k_dec_tans_gl (the class mask is learned), the next does not."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
import torch  # noqa: E402

mic = entry.load_package()
F = int(os.environ.get("FRAMES", "256")); S = 512
ct = np.fromfile(os.path.join(ROOT, "tests", "golden", "CT_512_512_image.bin"), dtype="<u2").reshape(S, S)
host = np.stack([np.roll(ct, i % 8, axis=1) for i in range(F)])
d_px = torch.from_numpy(host.view(np.int16)).cuda()
raw = host.nbytes
WORKED_MS = 0.1                      # a tANS decode kernel above this decoded streams (an empty class launch is ~0.005 ms)


def table_log(blob: bytes) -> int:
    off = 6 if blob[0] == 0xFF else 0
    return (blob[off] & 0xF) + 5


def run(passes):
    """one session, one encode + decode per entry of `passes` (the units' flag); figures of the last pass"""
    d_out = torch.empty_like(d_px)
    sess = mic.Session(F, S * S)
    try:
        used = []
        for flag in passes:
            units = mic.Session.make_units([(i * S * S, S, S, 65535, 2 | flag) for i in range(F)])
            sess.set_timing(True)
            sess.encode_enqueue(d_px.data_ptr(), units); te = sess.last_timings()
            d_blobs, offs, st, _ = sess.encode_finish()
            assert (st == 0).all(), st[:8]
            sess.decode_enqueue(d_blobs, offs, units, d_out.data_ptr()); td = sess.last_timings()
            assert (sess.decode_finish() == 0).all()
            tans = [(k, ms) for k, ms in td if k.startswith("k_dec_tans")]
            used.append((", ".join(k for k, ms in tans if ms > WORKED_MS) or "-", sum(ms for _, ms in tans)))
        assert torch.equal(d_out, d_px)
        first = torch.empty(int(offs[1]), dtype=torch.uint8, device="cuda")
        mic.device_copy(first.data_ptr(), d_blobs, int(offs[1]))
        b = first.cpu().numpy().tobytes()
        hdr = mic_gap_header_len(b) if passes[-1] else 0
        tl = table_log(b[hdr:])
        return int(offs[-1]), te, td, tl, hdr, used
    finally:
        sess.close()


def mic_gap_header_len(b: bytes) -> int:
    """bytes of mode || map in front of the FSE stream (the restatement of :178-256, for the encoder's two modes)"""
    if b[0] == 0:
        return 1
    n = b[1] | (b[2] << 8)
    if b[0] == 1:
        return 3 + 2 * n
    p = 5
    for _ in range(1, n):
        p += 3 if b[p] == 0xFF else 1
    return p


G = mic.MIC_HIP_GAP_REMOVAL
for name, passes in (("plain", [0, 0, 0]), ("gap", [G, G, G])):
    total, te, td, tl, hdr, used = run(passes)
    print(f"{name}: {F} frames {S}x{S}, ratio {raw / total:.3f} ({total / F:.0f} B/frame, map {hdr} B), tableLog {tl}")
    print(f"  tANS decode kernels that decoded (third pass): {used[-1][0]} ({used[-1][1]:.3f} ms)")
    for kname, ms in te + td:
        if ms > 0.02:
            print(f"  {kname:34s} {ms:8.3f} ms")
    enc = sum(ms for _, ms in te); dec = sum(ms for _, ms in td)
    print(f"  encode {enc:.3f} ms ({raw / enc / 1e6:.1f} GB/s)   decode {dec:.3f} ms ({raw / dec / 1e6:.1f} GB/s) (kernel time)")

# a session that has only seen plain CT batches meets a gap batch: its decode class mask is stale for one batch
total, te, td, tl, hdr, used = run([0, 0, 0, G, G])
print(f"gap after three plain batches on one session: first gap pass {used[3][0]} ({used[3][1]:.3f} ms), "
      f"next {used[4][0]} ({used[4][1]:.3f} ms)")
