"""NV12 frames against BGR frames, in ONE process (NV12.md).  Interleaved rounds, median of 5 (min - max), frames/s; planted weights
(tests/planted.py), default scales [1, 0.85, 0.7]; every frame is read from the handle's PINNED buffers:
  (1) vnect_infer against vnect_infer_nv12 (the frame crossing PCIe inside the call), at 368 x 368 and 1920 x 1080, fp32 and bf16;
  (2) runner.track_on_device with ahead 1, BGR against NV12, at 640 x 480 and 1920 x 1080, fp32 and bf16;
  (3) the same with source="resident": vnect_upload_frame against vnect_upload_frame_nv12 of the whole frame, one per frame.
    python3 tools/nv12_rate.py > profiles/nv12_rate.txt"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import planted  # noqa: E402
from vnect_amd import VNectEstimator, pixfmt, runner  # noqa: E402

ROUNDS = 5
N_INFER = 200
N_TRACK = 160
PRECS = ("fp32", "bf16")


def scenes(H, W):
    """Two frames, the person small on the left / large on the right, as NV12 and as the BGR frames the conversion makes of them."""
    nv = []
    for cy, cx, r in ((0.45 * H, 0.35 * W, 0.06 * H), (0.50 * H, 0.60 * W, 0.16 * H)):
        blobs = [(cy - 0.8 * r, cx, 0, 255.0), (cy + 0.9 * r, cx - 1.2 * r, 1, 255.0), (cy + 0.3 * r, cx + 1.5 * r, 2, 255.0)]
        nv.append(pixfmt.bgr_to_nv12(planted.scene(H, W, blobs, sigma=max(6.0, H / 80.0), seed=5)))
    return nv, [pixfmt.nv12_to_bgr(f) for f in nv]


class Clock:
    def __init__(self):
        self.t = 1.7e9

    def take(self, n):
        ts = [(self.t + 0.001 * k, self.t + 0.001 * k + 0.0002) for k in range(n)]
        self.t += 0.001 * n + 1.0
        return ts


def fill(est, H, W, imgs, fmt):
    bufs = [est.frame_buffer(H, W, b, pixel_format=fmt) for b in range(2)]
    for b in range(2):
        bufs[b][...] = imgs[b]
    return bufs


def infer_rate(est, H, W, imgs, fmt, n, clock):
    est.reset()
    bufs = fill(est, H, W, imgs, fmt)
    ts = clock.take(n)
    h = est.handle
    call = h.infer_nv12 if fmt == "nv12" else h.infer
    t0 = time.perf_counter()
    for k in range(n):
        call(bufs[k & 1], ts[k][0], ts[k][1])
    return n / (time.perf_counter() - t0)


def track_rate(est, H, W, imgs, fmt, n, clock, source="pinned"):
    est.reset()
    bufs = fill(est, H, W, imgs, fmt)
    ts = clock.take(n)
    t0 = time.perf_counter()
    for _ in runner.track_on_device(est, (bufs[k & 1] for k in range(n)), timestamps=ts, ahead=1, source=source, pixel_format=fmt):
        pass
    return n / (time.perf_counter() - t0)


def resident_rate(est, H, W, imgs, fmt, n, clock):
    """the whole frame uploaded into a resident slot per frame (vnect_upload_frame / vnect_upload_frame_nv12) while the previous computes"""
    return track_rate(est, H, W, imgs, fmt, n, clock, source="resident")


def report(tag, rates):
    for name, v in rates.items():
        v = sorted(v)
        print("  %-44s %-22s median %8.1f  (%8.1f - %8.1f) frames/s" % (tag, name, v[len(v) // 2], v[0], v[-1]))
    b, a = sorted(rates["bgr"])[ROUNDS // 2], sorted(rates["nv12"])[ROUNDS // 2]
    print("  %-44s nv12 / bgr             %.3f" % (tag, a / b))


def measure(fn, sizes, n):
    w = planted.weights(noise=1.0)
    clock = Clock()
    for prec in PRECS:
        est = VNectEstimator(weights=w, verbose=False, precision=prec)
        try:
            for H, W in sizes:
                nv, bgr = scenes(H, W)
                src = {"bgr": bgr, "nv12": nv}
                for fmt in src:                      # warm both paths
                    fn(est, H, W, src[fmt], fmt, 20, clock)
                rates = {"bgr": [], "nv12": []}
                for _ in range(ROUNDS):
                    for fmt in src:
                        rates[fmt].append(fn(est, H, W, src[fmt], fmt, n, clock))
                report("%s %d x %d" % (prec, W, H), rates)
        finally:
            est.close()


def main():
    print(__doc__.split("\n    python3")[0])
    print("(1) vnect_infer / vnect_infer_nv12 from the pinned buffers, %d frames per trial:" % N_INFER)
    measure(infer_rate, ((368, 368), (1080, 1920)), N_INFER)
    print("(2) runner.track_on_device, ahead 1, source pinned, %d frames per trial:" % N_TRACK)
    measure(track_rate, ((480, 640), (1080, 1920)), N_TRACK)
    print("(3) runner.track_on_device, ahead 1, source resident (an upload per frame, overlapping the previous frame), %d frames per trial:" % N_TRACK)
    measure(resident_rate, ((480, 640), (1080, 1920)), N_TRACK)


if __name__ == "__main__":
    main()
