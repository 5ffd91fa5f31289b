"""Orientation on the device against turning the frame oneself, in ONE process (ORIENTATION.md).  A 1920 x 1080 stored frame under
orientation 3 (the reference's T: the picture is 1080 wide and 1920 high) with a 400 x 600 person crop in the picture's coordinates,
synchronous calls, planted weights (tests/planted.py), default scales; the variants take turns in rounds of 20 frames until each has run
200 timed frames (one warm-up round each first), the scheme of tools/device_frame_rate.py.  frames/s = timed frames / summed time; the
do-it-yourself variant runs twice, and the A/A pair gives the spread of the call.
  (a) the oriented copy's own duration for that crop (device events around each launch, median of 200): device BGR, device NV12, pinned
      BGR -- each beside the unoriented copy of the SAME pixels, the stored rectangle the crop reads, by the copy code 0 launches;
  (b) synchronous est(tensor, orientation=3, rect) against est(torch.rot90(tensor, 3, (0, 1)).contiguous(), rect);
  (c) tracked, one frame at a time: the pinned loop with orientation=3 (the stored frame copied into the pinned buffer, the crop turned on
      the device) against transpose=True (np.rot90 on the host into the pinned buffer), and the device loop against rotate-then-submit.
torch is imported first (one HIP runtime in the process); the device frames are torch tensors.
    python3 tools/orient_rate.py > profiles/orient_rate.txt"""
import ctypes as C
import os
import sys
import time

import torch  # noqa: F401  (before vnect_amd: one HIP runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import devframe_ref as dr  # noqa: E402
from tests import orient_ref as orf  # noqa: E402
from tests import planted  # noqa: E402
from vnect_amd import VNectEstimator, _native, pixfmt  # noqa: E402

H, W, O = 1080, 1920, 3                      # the stored frame; its picture is (W, H) = 1920 high, 1080 wide
RECT = (340, 660, 400, 600)                  # in the picture's coordinates
ROUND, TIMED = 20, 200
PRECS = ("fp32", "bf16")


def scene():
    """the stored frame: a person in the PICTURE, turned back"""
    Ho, Wo = W, H
    cy, cx, r = RECT[1] + 0.5 * RECT[3], RECT[0] + 0.5 * RECT[2], 0.12 * Wo
    blobs = [(cy - 0.8 * r, cx, 0, 255.0), (cy + 0.9 * r, cx - 1.2 * r, 1, 255.0), (cy + 0.3 * r, cx + 1.5 * r, 2, 255.0)]
    pic = planted.scene(Ho, Wo, blobs, sigma=Wo / 80.0, seed=5)
    stored = np.ascontiguousarray(np.rot90(pic, 1))
    assert np.array_equal(orf.oriented(stored, O), pic)
    return stored


def run(variants, clock):
    spent = {k: 0.0 for k in variants}
    for rnd in range(1 + TIMED // ROUND):
        for name, f in variants.items():
            ts = [(clock[0] + 0.001 * k, clock[0] + 0.001 * k + 0.0002) for k in range(ROUND)]
            clock[0] += 1.0
            t0 = time.perf_counter()
            for t in ts:
                f(*t)
            if rnd:
                spent[name] += time.perf_counter() - t0
    return {k: TIMED / v for k, v in spent.items()}


def report(tag, rates, base, base2):
    spread = abs(rates[base] - rates[base2]) / rates[base]
    for name, v in rates.items():
        rel = v / rates[base] - 1.0
        note = "" if name in (base, base2) else ("  SLOWER than the spread" if rel < -spread else "  not slower than the spread")
        print("  %-6s %-52s %8.1f frames/s  %+6.2f %%%s" % (tag, name, v, 100 * rel, note))
    print("  %-6s A/A spread %.2f %%" % (tag, 100 * spread))


def kernels():
    P = orf.load_probe()
    P.op_time_copy.argtypes = [C.c_int] * 5 + [dr.i32p, C.c_int, C.POINTER(C.c_float)]
    ms = np.zeros(200, np.float32)
    msp = ms.ctypes.data_as(C.POINTER(C.c_float))
    stored = (C.c_int32 * 4)()
    orf.cpu_lib().orient_src_rect_c(O, H, W, *RECT, stored)           # the same pixels where they are stored: 600 x 400
    r, pr = np.asarray(RECT, np.int32), np.asarray(list(stored), np.int32)
    print("the copy kernels alone, crop %d x %d (stored: x %d, y %d, %d x %d), device events around each launch, median of 200 (min):"
          % (RECT[2], RECT[3], pr[0], pr[1], pr[2], pr[3]))
    for name, nv12, pinned in (("device BGR", 0, 0), ("device NV12", 1, 0), ("pinned BGR (over PCIe)", 0, 1)):
        for tag, o, rect in (("oriented", O, r), ("unoriented", 0, pr)):
            rc = P.op_time_copy(nv12, pinned, o, H, W, rect.ctypes.data_as(dr.i32p), len(ms), msp)
            assert rc == 0, (name, tag, rc)
            print("  %-40s %7.1f us  (%7.1f)" % (tag + ", " + name, 1e3 * float(np.median(ms)), 1e3 * float(ms.min())))


def main():
    print(__doc__.split("\n    python3")[0])
    w = planted.weights(noise=1.0)
    stored = scene()
    t = torch.from_numpy(stored).cuda()
    torch.cuda.synchronize()
    clock = [1.7e9]
    kernels()
    for prec in PRECS:
        est = VNectEstimator(weights=w, verbose=False, precision=prec)
        try:
            h = est.handle

            def diy(a, b):
                return est(torch.rot90(t, 3, (0, 1)).contiguous(), timestamp=(a, b), rect=RECT)

            def oriented(a, b):
                return est(t, timestamp=(a, b), rect=RECT, orientation=O)
            want, got = diy(clock[0], clock[0]), None
            est.reset()
            got = oriented(clock[0], clock[0])
            assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])     # the same bits before any timing
            est.reset()
            clock[0] += 1.0
            print("(b) synchronous, %s:" % prec)
            report(prec, run({"est(torch.rot90(t, 3).contiguous(), rect) (A)": diy, "est(torch.rot90(t, 3).contiguous(), rect) (A')": diy,
                              "est(t, orientation=3, rect)": oriented}, clock), "est(torch.rot90(t, 3).contiguous(), rect) (A)",
                   "est(torch.rot90(t, 3).contiguous(), rect) (A')")
            # (c) tracked: stream 0 takes turned frames (orientation 0), stream 1 stored frames under orientation 3
            est.reset()
            est._orient(0)
            h.track_begin(0, W, H, RECT)
            est._orient(O)
            h.track_begin(1, W, H, RECT)
            est._orient(0)
            pin = [h.frame_buffer(b, H, W).reshape(-1) for b in range(2)]
            turned, plain = pin[0].reshape(W, H, 3), pin[1].reshape(H, W, 3)

            def host_rot(a, b):
                turned[...] = np.rot90(stored, 3)
                h.submit_tracked_pinned(0, 0, 3 * H, a, b)
                h.collect_tracked()

            def dev_orient(a, b):
                plain[...] = stored
                h.submit_tracked_pinned(1, 1, 3 * W, a, b)
                h.collect_tracked()
            print("(c) tracked from the pinned buffers, %s:" % prec)
            report(prec, run({"transpose=True: np.rot90 on the host (A)": host_rot, "transpose=True: np.rot90 on the host (A')": host_rot,
                              "orientation=3: the crop turned on the device": dev_orient}, clock), "transpose=True: np.rot90 on the host (A)",
                   "transpose=True: np.rot90 on the host (A')")
            whole = _native.device_frame(t, "bgr")
            stream = torch.cuda.current_stream().cuda_stream

            def dev_rot(a, b):
                r = torch.rot90(t, 3, (0, 1)).contiguous()
                h.submit_tracked_device(0, _native.device_frame(r, "bgr"), a, b, stream)
                h.collect_tracked()

            def dev_o(a, b):
                h.submit_tracked_device(1, whole, a, b, stream)
                h.collect_tracked()
            print("(c) tracked from device memory, %s:" % prec)
            report(prec, run({"torch.rot90(t, 3).contiguous(), then submit (A)": dev_rot, "torch.rot90(t, 3).contiguous(), then submit (A')": dev_rot,
                              "submit under orientation 3": dev_o}, clock), "torch.rot90(t, 3).contiguous(), then submit (A)",
                   "torch.rot90(t, 3).contiguous(), then submit (A')")
        finally:
            est.close()


if __name__ == "__main__":
    main()
