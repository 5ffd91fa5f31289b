"""The preview's cost (PREVIEW.md), in ONE process on one MI355X.  1920 x 1080 frames (the scene and the 400 x 600 person rect of
profiles/device_frame_rate.txt) and their 3840 x 2160 pixel-doubled twins, packed BGR and NV12, stored under code 0 and code 3, at the
default factor (1024 on the longer side); 21 joints spread over the rect.
  (a) the kernel alone: device events around each launch (the kernel probe, which makes a frame of the size itself; median, min of 200);
      also at factors 0.25, 1.0 (the copy) and 1.7 on the 1920 x 1080 frame, with the time per output pixel;
  (b) vnect_preview_device, wall clock of the synchronous call (validation, event, launch, copy, wait): into device memory and into
      pinned host memory (vnect_frame_buffer);
  (c) what a caller had before: device -> host copy of the frame, render.draw_limbs_2d_exact, render.resize_u8_exact (numpy);
  (d) the tracked device loop, one frame at a time (submit + collect), fp32 and bf16, the 400 x 600 crop: preview=False twice (the
      A / A' pair gives the run's own spread) against preview=True, packed BGR and NV12;
  (e) runner.track_on_device with ahead=1 on a lanes=2 handle, where the preview's launch and copy can overlap the next frame.
Within each of (a), (b) + (c), (d) and (e) the variants take turns in rounds of 20 until each has run 200 timed frames (one warm-up
round each first).  us = summed time / timed calls; frames/s = timed frames / summed time.  The device memory comes from the probes'
allocator: no torch, one HIP runtime.
    python3 tools/preview_rate.py > profiles/preview_rate.txt"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import devframe_ref as dr  # noqa: E402
from tests import preview_ref as pref  # noqa: E402
from tools.device_frame_rate import RECT, H, W, Device, scene  # noqa: E402
from tests import planted  # noqa: E402
from vnect_amd import VNectEstimator, _native, pixfmt, render, runner  # noqa: E402

ROUND, TIMED = 20, 200


def joints(rect):
    x, y, w, h = rect
    rs = np.random.RandomState(3)
    return np.stack([rs.uniform(y, y + h, 21), rs.uniform(x, x + w, 21)], 1)


def turned(rect, o, Hs, Ws):
    """the stored frame's rect in the oriented picture of code o (0 or 3: np.rot90(frame, 3))"""
    x, y, w, h = rect
    return rect if o == 0 else (Hs - y - h, x, h, w)


def rounds(variants, per_round=ROUND):
    """variants: name -> f(round number) running `per_round` calls.  Interleaved rounds -> name -> seconds per call"""
    spent = {k: 0.0 for k in variants}
    for rnd in range(1 + TIMED // ROUND):
        for name, f in variants.items():
            t0 = time.perf_counter()
            f(rnd)
            if rnd:
                spent[name] += time.perf_counter() - t0
    return {k: v / TIMED for k, v in spent.items()}


def spread_lines(prec, r, base, base2, ref_of):
    spread = abs(r[base] - r[base2]) / r[base]
    for name, sec in r.items():
        ref = r[ref_of(name)]
        rel = ref / sec - 1.0
        note = "" if "preview=False" in name else ("  %+6.1f us per frame; %s" % (1e6 * (sec - ref), "slower than the spread" if rel < -spread else "within the spread"))
        print("  %-6s %-32s %8.1f frames/s  %+6.2f %%%s" % (prec, name, 1.0 / sec, 100 * rel, note))
    print("  %-6s A/A' spread %.2f %%" % (prec, 100 * spread))


def main():
    print(__doc__.split("\n    python3")[0])
    P = pref.probe_lib()
    P.pp_time.restype, P.pp_time.argtypes = C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_float), pref.i32p]
    samples, shapes = {}, {}

    def kernel(fmt, Hs, Ws, o, key, f=0.0):
        def go(rnd):
            ms, hw = np.zeros(ROUND, np.float32), np.zeros(2, np.int32)
            rc = P.pp_time(fmt, Hs, Ws, o, f, ROUND, ms.ctypes.data_as(C.POINTER(C.c_float)), hw.ctypes.data_as(pref.i32p))
            assert rc == 0, rc
            shapes[key] = (int(hw[1]), int(hw[0]))
            if rnd:
                samples.setdefault(key, []).extend(float(v) for v in ms)
        return go
    va = {}
    for Hs, Ws in ((H, W), (2 * H, 2 * W)):
        for fmt, name in ((0, "packed BGR"), (2, "NV12")):
            for o in (0, 3):
                key = "%4d x %4d %-10s code %d" % (Ws, Hs, name, o)
                va[key] = kernel(fmt, Hs, Ws, o, key)
    for f in (0.25, 1.0, 1.7):      # other factors (1.0 is the copy): does a fetched tap cost more where neighbours do not share it?
        key = "%4d x %4d %-10s code 0 f = %.2f" % (W, H, "packed BGR", f)
        va[key] = kernel(0, H, W, 0, key, f)
    rounds(va)
    print("(a) the preview kernel alone, default factor unless given, device events around each launch, median of %d (min), and ns per output pixel:" % TIMED)
    for key, ms in samples.items():
        px = shapes[key][0] * shapes[key][1]
        print("  %-38s -> %4d x %4d   %7.1f us  (%7.1f)   %6.3f ns/px" % (key, shapes[key][0], shapes[key][1], 1e3 * np.median(ms), 1e3 * min(ms), 1e6 * np.median(ms) / px))

    nv, bgr = scene()
    frames = {(H, W): (nv, bgr)}
    big = np.repeat(np.repeat(bgr, 2, 0), 2, 1)
    frames[(2 * H, 2 * W)] = (pixfmt.bgr_to_nv12(big), big)
    dev = Device()
    w = planted.weights(noise=1.0)
    clock = [1.7e9]
    try:
        est = VNectEstimator(weights=w, verbose=False)    # (a handle with pinned frame buffers)
        h = est._h
        try:
            variants = {}
            pinned = h.frame_buffer(0, 1024, 1024)
            for (Hs, Ws), (nvf, bgrf) in frames.items():
                rect = tuple((Hs // H) * v for v in RECT)
                pb = dev.put(bgrf)
                for fmt, arr in (("bgr", dr.FakeCuda(pb, (Hs, Ws, 3))), ("nv12", dr.FakeCuda(dev.put(nvf), (Hs * 3 // 2, Ws)))):
                    frame = _native.device_frame(arr, fmt)
                    for o in (0, 3):
                        r = turned(rect, o, Hs, Ws)
                        j2, spec = joints(r), _native.preview_spec()
                        h.set_orientation(o)
                        dh, dw = h.preview_size(frame, spec)
                        out = dev.put(np.zeros(dh * dw * 3, np.uint8))
                        for where, ptr in (("device", out), ("pinned host", pinned.ctypes.data)):
                            def call(rnd, frame=frame, spec=spec, ptr=ptr, dw=dw, j2=j2, r=r, o=o):
                                if h.orientation != o:
                                    h.set_orientation(o)
                                for _ in range(ROUND):
                                    h.preview_device(frame, spec, ptr, 3 * dw, j2, r, None, None, _native.STREAM_SYNCED)
                            variants["(b) %4d x %4d %-4s code %d -> %s" % (Ws, Hs, fmt, o, where)] = call
                host = np.empty_like(bgrf)

                def before(rnd, pb=pb, host=host, rect=rect):
                    for _ in range(ROUND):
                        assert dev.L.ip_d2h(host.ctypes.data, pb, host.size) == 0
                        render.resize_u8_exact(render.draw_limbs_2d_exact(host, joints(rect), pref.R.PARENTS, rect), None)
                variants["(c) %4d x %4d bgr  download, numpy draw and resize" % (Ws, Hs)] = before
            print("(b) vnect_preview_device, wall clock of the synchronous call, and (c) what a caller had before, %d timed calls each in rounds of %d:" % (TIMED, ROUND))
            for name, sec in rounds(variants).items():
                print("  %-56s %9.1f us" % (name, 1e6 * sec))
        finally:
            est.close()

        nvf, bgrf = frames[(H, W)]
        for prec in ("fp32", "bf16"):
            est = VNectEstimator(weights=w, verbose=False, precision=prec)
            try:
                h = est.handle
                style, spec = _native.overlay_style(parents=est.joint_parents), _native.preview_spec()
                legs = {"preview=False packed BGR (A)": ("bgr", False), "preview=False packed BGR (A')": ("bgr", False), "preview=True  packed BGR": ("bgr", True),
                        "preview=False NV12": ("nv12", False), "preview=True  NV12": ("nv12", True)}
                est.reset()
                h.track_begin(0, H, W, RECT)

                def tracked(fmt, pv):
                    f = _native.device_frame(dr.FakeCuda(dev.put(bgrf), (H, W, 3)) if fmt == "bgr" else dr.FakeCuda(dev.put(nvf), (H * 3 // 2, W)), fmt)

                    def go(rnd):
                        ts = [(clock[0] + 0.001 * k, clock[0] + 0.001 * k + 0.0002) for k in range(ROUND)]
                        clock[0] += 1.0
                        for a, b in ts:
                            if pv:
                                h.submit_tracked_device_preview(0, f, a, b, 0, style, spec)
                            else:
                                h.submit_tracked_device(0, f, a, b, 0)
                            h.collect_tracked()
                            if pv:
                                h.result_preview()
                    return go
                r = rounds({k: tracked(fmt, pv) for k, (fmt, pv) in legs.items()})
                print("(d) the tracked device loop, one frame at a time, %s (preview=True: 1024 x 576, fetched with vnect_result_preview and copied):" % prec)
                spread_lines(prec, r, "preview=False packed BGR (A)", "preview=False packed BGR (A')", lambda n: "preview=False NV12" if "NV12" in n else "preview=False packed BGR (A)")
            finally:
                est.close()

        for prec in ("fp32", "bf16"):
            est = VNectEstimator(weights=w, verbose=False, precision=prec, lanes=2)
            try:
                arr = dr.FakeCuda(dev.put(bgrf), (H, W, 3))

                def ahead(pv):
                    def go(rnd):
                        ts = [(clock[0] + 0.001 * k, clock[0] + 0.001 * k + 0.0002) for k in range(ROUND)]
                        clock[0] += 1.0
                        n = sum(1 for _ in runner.track_on_device(est, [arr] * ROUND, rect=RECT, timestamps=ts, ahead=1, source="device", preview=pv))
                        assert n == ROUND
                    return go
                r = rounds({"preview=False (A)": ahead(False), "preview=False (A')": ahead(False), "preview=True": ahead(True)})
                print("(e) runner.track_on_device, ahead=1, lanes=2, packed BGR, %s (each round is one loop of %d frames, its track_begin included):" % (prec, ROUND))
                spread_lines(prec, r, "preview=False (A)", "preview=False (A')", lambda n: "preview=False (A)")
            finally:
                est.close()
    finally:
        dev.close()


if __name__ == "__main__":
    main()
