"""The overlay's cost (OVERLAY.md), in ONE process.  1920 x 1080 frames with a 400 x 600 person crop, planted weights (tests/planted.py),
default scales, the geometry of profiles/device_frame_rate.txt; the joints and the rect drawn are those of one tracked frame of the scene.
  (a) the draw alone: the overlay kernel's duration, device events around each of 200 launches (the kernel probe; median and min) -- its
      inputs as kernel arguments (vnect_draw_device's form), in device memory, and in device-mapped pinned host memory where the tracked
      form reads them (the result ring's slots) -- and the wall time of the synchronous vnect_draw_device call;
  (b) the tracked device loop, one frame at a time (submit + collect), draw=False twice (the A/A pair gives the run's own spread) against
      draw=True on packed BGR and on NV12 frames, fp32 and bf16;
  (c) what a caller has without it: device -> host copy of the frame, render.draw_limbs_2d (PIL), host -> device copy.
The variants of (b), and the two calls of (a) and (c), take turns in rounds of 20 until each has run 200 timed frames (one warm-up round
each first).  frames/s = timed frames / summed time.  The device memory comes from the probes' allocator: no torch, one HIP runtime.
    python3 tools/overlay_rate.py > profiles/overlay_rate.txt"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import devframe_ref as dr  # noqa: E402
from tests import overlay_ref as oref  # noqa: E402
from tests import planted  # noqa: E402
from tools.device_frame_rate import RECT, H, W, Device, scene  # noqa: E402
from vnect_amd import VNectEstimator, _native, render  # noqa: E402

ROUND, TIMED = 20, 200
PRECS = ("fp32", "bf16")


def run(variants, clock):
    """variants: name -> f(t2d, t3d) running one synchronous frame.  Interleaved rounds -> name -> frames/s"""
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


def main():
    print(__doc__.split("\n    python3")[0])
    w = planted.weights(noise=1.0)
    nv, bgr = scene()
    dev = Device()
    P = oref.probe_lib()
    P.op_time_draw.restype = C.c_int
    P.op_time_draw.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, oref.f64p, oref.i32p,
                               C.c_int, C.c_int, C.POINTER(C.c_float)]
    clock = [1.7e9]
    try:
        rgb_planes = np.ascontiguousarray(bgr[..., ::-1].transpose(2, 0, 1))

        def packed():
            return dr.FakeCuda(dev.put(bgr), (H, W, 3))

        def nv12():
            return dr.FakeCuda(dev.put(nv), (H * 3 // 2, W))

        joints = used = None
        loops = {}
        for prec in PRECS:
            est = VNectEstimator(weights=w, verbose=False, precision=prec)
            try:
                h = est.handle
                style = _native.overlay_style(parents=est.joint_parents)
                frames = {"draw=False packed BGR (A)": (packed(), "bgr", None), "draw=False packed BGR (A')": (packed(), "bgr", None),
                          "draw=True  packed BGR": (packed(), "bgr", style), "draw=False NV12": (nv12(), "nv12", None), "draw=True  NV12": (nv12(), "nv12", style)}
                est.reset()
                h.track_begin(0, H, W, RECT)

                def tracked(f, st):
                    def go(a, b):
                        if st is None:
                            h.submit_tracked_device(0, f, a, b, 0)
                        else:
                            h.submit_tracked_device_draw(0, f, a, b, 0, st)
                        return h.collect_tracked()
                    return go
                v = {k: tracked(_native.device_frame(a, fmt), st) for k, (a, fmt, st) in frames.items()}
                if joints is None:                       # one tracked frame of the scene gives the joints and the rect every leg draws
                    _, joints, _, used = v["draw=False packed BGR (A)"](clock[0] - 1.0, clock[0] - 1.0 + 0.0002)
                loops[prec] = run(v, clock)
            finally:
                est.close()
        print("(b) the tracked device loop, one frame at a time:")
        base, base2 = "draw=False packed BGR (A)", "draw=False packed BGR (A')"
        for prec in PRECS:
            r = loops[prec]
            spread = abs(r[base] - r[base2]) / r[base]
            for name, val in r.items():
                ref = r["draw=False NV12"] if "NV12" in name else r[base]
                rel = val / ref - 1.0
                us = 1e6 / val - 1e6 / ref
                note = "" if name.startswith("draw=False") else ("  %+6.1f us per frame; %s" % (us, "slower than the spread" if rel < -spread else "within the spread"))
                print("  %-6s %-30s %8.1f frames/s  %+6.2f %%%s" % (prec, name, val, 100 * rel, note))
            print("  %-6s A/A spread %.2f %%" % (prec, 100 * spread))

        print("(a) the overlay kernel alone, %d x %d frame, 20 limbs and the %d x %d rect of a tracked frame, device events around each launch, median of 200 (min):"
              % (W, H, used[2], used[3]))
        j = np.ascontiguousarray(joints, np.float64)
        r4 = np.asarray(used, np.int32)
        ms = np.zeros(200, np.float32)
        pb, pp, pn = dev.put(bgr), dev.put(rgb_planes), dev.put(nv)
        rows = [("packed BGR", pb, None, 0, (3 * W, 3, 1)), ("planar RGB", pp, None, 1, (W, 1, H * W)), ("NV12", pn, pn + H * W, 2, (W, 1, 0))]
        for name, p, uv, fmt, (sy, sx, sc) in rows:
            for tracked_form, where in ((0, "kernel arguments"), (1, "device memory"), (2, "pinned host memory (the ring slot's)")):
                rc = P.op_time_draw(p, uv, fmt, H, W, sy, sx, sc, W, j.ctypes.data_as(oref.f64p), r4.ctypes.data_as(oref.i32p), tracked_form, len(ms),
                                    ms.ctypes.data_as(C.POINTER(C.c_float)))
                assert rc == 0, (name, rc)
                print("  %-12s inputs in %-38s %7.1f us  (%7.1f)" % (name, where, 1e3 * float(np.median(ms)), 1e3 * float(ms.min())))

        print("(a) / (c) per call, wall clock of a synchronous call, packed BGR:")
        hp = _native.Handle([1.0], preprocess_only=True)
        try:
            target = dev.put(bgr)
            df = _native.device_frame(dr.FakeCuda(target, (H, W, 3)))
            host = np.empty((H, W, 3), np.uint8)
            parents = VNectEstimator.joint_parents

            def draw_device(a, b):
                hp.draw_device(df, j, used, None, None, _native.STREAM_SYNCED)

            def today(a, b):
                assert dev.L.ip_d2h(host.ctypes.data, target, host.size) == 0
                out = render.draw_limbs_2d(host, j, parents, used)
                assert dev.L.ip_h2d(target, out.ctypes.data, out.size) == 0
            r = run({"vnect_draw_device": draw_device, "download + render.draw_limbs_2d + upload": today}, clock)
            for name, val in r.items():
                print("  %-44s %9.1f calls/s  %9.1f us per call" % (name, val, 1e6 / val))
        finally:
            hp.close()
    finally:
        dev.close()


if __name__ == "__main__":
    main()
