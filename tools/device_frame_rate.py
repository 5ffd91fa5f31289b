"""Frames in device memory against the pinned-buffer call, in ONE process (DEVICE_FRAMES.md).  1920 x 1080 frames with a 400 x 600 person
crop, synchronous calls, planted weights (tests/planted.py), default scales; the variants take turns in rounds of 20 frames until each has
run 200 timed frames (one warm-up round each first), the scheme of bench.py's call-surface leg.  frames/s = timed frames / summed time.
  untracked: vnect_infer of the crop cut out of the pinned buffer (twice: the A/A pair gives the spread) against vnect_infer_device with
             the same rect from packed BGR, planar RGB and NV12 frames in device memory;
  tracked:   vnect_submit_tracked_pinned + collect (twice) against vnect_submit_tracked_device + collect from the same three.
Then the copy kernels' own durations for that crop, device events around each launch (the kernel probe; median of 200).
The device memory comes from the probe's allocator: no torch, one HIP runtime.
    python3 tools/device_frame_rate.py > profiles/device_frame_rate.txt"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from tests import devframe_ref as dr  # noqa: E402
from tests import planted  # noqa: E402
from vnect_amd import VNectEstimator, _native, pixfmt  # noqa: E402

H, W = 1080, 1920
RECT = (700, 240, 400, 600)
ROUND, TIMED = 20, 200
PRECS = ("fp32", "bf16")


def scene():
    cy, cx, r = 0.50 * H, 0.47 * W, 0.12 * H
    blobs = [(cy - 0.8 * r, cx, 0, 255.0), (cy + 0.9 * r, cx - 1.2 * r, 1, 255.0), (cy + 0.3 * r, cx + 1.5 * r, 2, 255.0)]
    nv = pixfmt.bgr_to_nv12(planted.scene(H, W, blobs, sigma=H / 80.0, seed=5))
    return nv, pixfmt.nv12_to_bgr(nv)            # the BGR frame is the NV12 frame's conversion: every variant sees the same pixels


class Device:
    def __init__(self):
        self.L = dr.load_probe()
        self.L.ip_time_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, dr.i32p, C.c_int,
                                        C.c_int, C.POINTER(C.c_float)]
        self.ptrs = []

    def put(self, a):
        a = np.ascontiguousarray(a).reshape(-1)
        p = C.c_void_p()
        assert self.L.ip_alloc(len(a), C.byref(p)) == 0
        assert self.L.ip_h2d(p, a.ctypes.data, len(a)) == 0
        self.ptrs.append(p.value)
        return p.value

    def close(self):
        for p in self.ptrs:
            self.L.ip_free(p)


def device_frames(dev, nv, bgr):
    """name -> (device array, pixel_format)"""
    rgb_planes = np.ascontiguousarray(bgr[..., ::-1].transpose(2, 0, 1))
    return {"device packed BGR": (dr.FakeCuda(dev.put(bgr), (H, W, 3)), "bgr"),
            "device planar RGB": (dr.FakeCuda(dev.put(rgb_planes), (H, W, 3), (W, 1, H * W)), "rgb"),
            "device NV12": (dr.FakeCuda(dev.put(nv), (H * 3 // 2, W)), "nv12")}


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


def report(tag, rates, base, base2):
    spread = abs(rates[base] - rates[base2]) / rates[base]
    for name, v in rates.items():
        rel = v / rates[base] - 1.0
        note = "" if name in (base, base2) else ("  slower than the spread" if rel < -spread else "  not slower than the spread")
        print("  %-10s %-34s %8.1f frames/s  %+6.2f %%%s" % (tag, name, v, 100 * rel, note))
    print("  %-10s A/A spread %.2f %%" % (tag, 100 * spread))


def main():
    print(__doc__.split("\n    python3")[0])
    w = planted.weights(noise=1.0)
    nv, bgr = scene()
    dev = Device()
    clock = [1.7e9]
    try:
        frames = device_frames(dev, nv, bgr)
        for prec in PRECS:
            est = VNectEstimator(weights=w, verbose=False, precision=prec)
            try:
                h = est.handle
                pin = est.frame_buffer(H, W, 0)
                pin[...] = bgr
                x, y, cw, ch = RECT
                crop = pin[y:y + ch, x:x + cw]
                dfs = {k: _native.device_frame(a, fmt, RECT) for k, (a, fmt) in frames.items()}
                est.reset()
                v = {"pinned vnect_infer (A)": lambda a, b: h.infer(crop, a, b), "pinned vnect_infer (A')": lambda a, b: h.infer(crop, a, b)}
                for k, f in dfs.items():
                    v[k] = (lambda f: lambda a, b: h.infer_device(f, a, b, 0))(f)
                print("untracked, %s:" % prec)
                report(prec, run(v, clock), "pinned vnect_infer (A)", "pinned vnect_infer (A')")
                # tracked: the box lives on the device; one frame at a time
                whole = {k: _native.device_frame(a, fmt) for k, (a, fmt) in frames.items()}
                est.reset()
                h.track_begin(0, H, W, RECT)

                def pinned(a, b):
                    h.submit_tracked_pinned(0, 0, 3 * W, a, b)
                    h.collect_tracked()

                def tracked(f):
                    def go(a, b):
                        h.submit_tracked_device(0, f, a, b, 0)
                        h.collect_tracked()
                    return go
                v = {"pinned tracked (A)": pinned, "pinned tracked (A')": pinned}
                for k, f in whole.items():
                    v[k + " tracked"] = tracked(f)
                print("tracked, %s:" % prec)
                report(prec, run(v, clock), "pinned tracked (A)", "pinned tracked (A')")
            finally:
                est.close()
        print("the copy kernels alone, crop %d x %d of the %d x %d frame, device events around each launch, median of 200 (min):" % (RECT[2], RECT[3], W, H))
        r = np.asarray(RECT, np.int32)
        ms = np.zeros(200, np.float32)
        rows = [("packed BGR", frames["device packed BGR"][0], 0, (3 * W, 3, 1), 0), ("planar RGB", frames["device planar RGB"][0], 1, (W, 1, H * W), 0),
                ("packed BGR, generic kernel", frames["device packed BGR"][0], 0, (3 * W, 3, 1), 1), ("NV12", frames["device NV12"][0], 2, (W, 1, 1), 0)]
        for name, a, fmt, (sy, sx, sc), generic in rows:
            p = a.__cuda_array_interface__["data"][0]
            rc = dev.L.ip_time_copy(p, p + H * W if fmt == 2 else None, fmt, H, W, sy, sx, sc, W, r.ctypes.data_as(dr.i32p), generic, len(ms),
                                    ms.ctypes.data_as(C.POINTER(C.c_float)))
            assert rc == 0, (name, rc)
            print("  %-30s %7.1f us  (%7.1f)" % (name, 1e3 * float(np.median(ms)), 1e3 * float(ms.min())))
    finally:
        dev.close()


if __name__ == "__main__":
    main()
