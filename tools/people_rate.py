"""People mode's rate (PEOPLE.md), in ONE process: P persons of one video, frames in device memory (packed BGR), planted weights
(tests/planted.py), default scales, lanes=3.  Three ways of doing the same work:
  many      the way without people mode: one vnect_submit_tracked_device per person and frame on a plain handle, the frame given P times
            (what runner.track_many_on_device(est, [frames] * P, ...) does), no draw;
  unpaired  vnect_submit_people_device on a people handle with pair = 0: one submit per frame, one conv stack per person;
  paired    the same with pair = 1: persons (0, 1) and (2, 3) share a conv stack.
P = 2 and 4; 640 x 480 and 1920 x 1080; fp32 and bf16; synchronous (a frame's P results collected before the next submit) and ahead 1 (the
next frame submitted first, where the in-flight limits allow: `depth` is the number of video frames really kept in flight; `many` keeps
two SUBMITS in flight, as track_many_on_device(ahead=1) does).  The variants of one (size, precision) take turns in 5 rounds of 40 frames
after one warm-up round; frames/s = video frames / time, the median of the 5 rounds.  Every person's results are the same bits in all
three ways (tests/test_gpu_people.py).  The device memory comes from the probes' allocator: no torch, one HIP runtime.
    python3 tools/people_rate.py > profiles/people_rate.txt"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import devframe_ref as dr  # noqa: E402
from tests import planted  # noqa: E402
from tools.device_frame_rate import Device  # noqa: E402
from vnect_amd import VNectEstimator, _native  # noqa: E402

ROUNDS, FRAMES = 5, 40
SIZES = ((480, 640), (1080, 1920))
PRECS = ("fp32", "bf16")
CENTRES = [(0.32, 0.26), (0.64, 0.70), (0.36, 0.74), (0.70, 0.30)]
LANES = 3


def scene(H, W):
    m = min(H, W)
    blobs = []
    for fy, fx in CENTRES:
        cy, cx, r = H * fy, W * fx, 0.08 * m
        blobs += [(cy - 0.8 * r, cx, 0, 255.0), (cy + 0.9 * r, cx - 1.2 * r, 1, 255.0), (cy + 0.3 * r, cx + 1.5 * r, 2, 255.0)]
    return planted.scene(H, W, blobs, sigma=m / 40.0, seed=5)


def rects(H, W, P):
    out = []
    for fy, fx in CENTRES[:P]:
        x0, y0 = max(int(W * (fx - 0.2)), 0), max(int(H * (fy - 0.25)), 0)
        out.append([x0, y0, min(int(W * 0.4), W - x0), min(int(H * 0.5), H - y0)])
    return out


def many(h, f, P, depth):
    """one submit per person; `depth` submits in flight"""
    def go(stamps):
        flying = 0
        for t in stamps:
            for p in range(P):
                h.submit_tracked_device(p, f, t, t + 0.0002, 0)
                flying += 1
                while flying >= depth:
                    h.collect_tracked()
                    flying -= 1
        while flying:
            h.collect_tracked()
            flying -= 1
    return go


def people(h, f, P, depth):
    """one submit per frame; `depth` frames in flight"""
    def go(stamps):
        flying = 0
        for t in stamps:
            h.submit_people_device(P, f, t, t + 0.0002, 0)
            flying += 1
            while flying >= depth:
                for _ in range(P):
                    h.collect_tracked()
                flying -= 1
        while flying:
            for _ in range(P):
                h.collect_tracked()
            flying -= 1
    return go


def main():
    print(__doc__.split("\n    python3")[0])
    w = planted.weights(noise=1.0)
    dev = Device()
    clock = [1.7e9]
    limit = max(LANES, 2)
    try:
        for H, W in SIZES:
            frame = _native.device_frame(dr.FakeCuda(dev.put(scene(H, W)), (H, W, 3)))
            for prec in PRECS:
                ests = {"many": VNectEstimator(weights=w, verbose=False, precision=prec, lanes=LANES),
                        "unpaired": VNectEstimator(weights=w, verbose=False, precision=prec, lanes=LANES, people=4, pair_people=False),
                        "paired": VNectEstimator(weights=w, verbose=False, precision=prec, lanes=LANES, people=4, pair_people=True)}
                try:
                    variants = {}
                    for P in (2, 4):
                        for ahead in (0, 1):
                            for way, est in ests.items():
                                units = P if way != "paired" else (P + 1) // 2
                                if way == "many":
                                    depth = min(ahead, limit - 1) + 1
                                    run = many(est.handle, frame, P, depth)
                                else:
                                    depth = max(0, min(ahead, limit // units - 1, 8 // P - 1)) + 1
                                    run = people(est.handle, frame, P, depth)
                                variants[(P, ahead, way)] = (est, run, depth)
                    rates = {k: [] for k in variants}
                    for rnd in range(1 + ROUNDS):
                        for key, (est, run, depth) in variants.items():
                            P = key[0]
                            h = est.handle
                            est.reset()
                            if key[2] == "many":
                                for p, r in enumerate(rects(H, W, P)):
                                    h.track_begin(p, H, W, r)
                            else:
                                h.people_begin(P, H, W, rects(H, W, P))
                            stamps = [clock[0] + 0.001 * k for k in range(FRAMES)]
                            clock[0] += 1.0
                            t0 = time.perf_counter()
                            run(stamps)
                            dt = time.perf_counter() - t0
                            if rnd:
                                rates[key].append(FRAMES / dt)
                    print("%d x %d, %s, lanes=%d: video frames/s, median of %d rounds (min .. max)" % (W, H, prec, LANES, ROUNDS))
                    for P in (2, 4):
                        for ahead in (0, 1):
                            base = float(np.median(rates[(P, ahead, "many")]))
                            for way in ("many", "unpaired", "paired"):
                                r = rates[(P, ahead, way)]
                                med = float(np.median(r))
                                print("  P=%d %-11s %-9s depth %d  %8.1f  (%8.1f .. %8.1f)  %+6.1f %% vs many" %
                                      (P, "synchronous" if not ahead else "ahead 1", way, variants[(P, ahead, way)][2], med, min(r), max(r), 100 * (med / base - 1)))
                finally:
                    for e in ests.values():
                        e.close()
    finally:
        dev.close()


if __name__ == "__main__":
    main()
